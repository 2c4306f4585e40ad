"""The case table of the flat Adam step (mal_amd.optim.FlatAdam, mal_amd/csrc/mal_adam.hip), importable without a device.
Shared by tests/test_flat_adam_cases.py (CPU: the restatement against torch, the plan, refusals, checkpoints) and
tests/test_gpu_flat_adam.py (GPU).

Chunk sizes: one element, sizes around the four-float vector (3, 4, 5), around a wavefront (63, 64, 65), a partial tile
(255, 1025) and one past two tiles of 2048 elements (4099), in five orderings: "mixed" alone puts chunks at every offset
residue modulo 4, and between them the orderings put the two-tile chunk at every residue (the CPU test proves both)."""
import torch

SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 1025, 4099)
ORDERINGS = {
    "ascending": (1, 3, 4, 5, 63, 64, 65, 255, 1025, 4099),    # offsets 0 1 4 8 13 76 140 205 460 1485: residues 0 1 0 0 1 0 0 1 0 1
    "mixed": (4099, 3, 1025, 1, 5, 255, 64, 63, 65, 4),        # offsets 0 4099 4102 5127 5128 5133 5388 5452 5515 5580: 0 3 2 3 0 1 0 0 3 0
    "long_at_1": (1, 4099, 1025, 3, 255, 65, 5, 64, 63, 4),    # the chunk longer than two tiles at residue 1 ...
    "long_at_2": (5, 1, 4099, 255, 1025, 3, 65, 64, 63, 4),    # ... at residue 2 ...
    "long_at_3": (3, 4099, 1, 1025, 255, 65, 5, 64, 63, 4),    # ... and at residue 3
}
TILE, THREADS, MAX_BLOCKS, WINDOW = 2048, 256, 2048, 256  # kAdamTile, kAdamThreads, kAdamMaxBlocks, kAdamWindow (mal_adam.hip)

# the margins of the restatement over torch.optim.Adam, both as L2-relative distances from the fp64 recurrence, measured on
# the CPU over GATE_CASES (tests/test_flat_adam_cases.py prints them): the largest ratio seen, and the gate = that x 1.25
MEASURED_RATIO = {"update": 1.0027, "m": 1.2016, "v": 1.0583}
GATE_RATIO = {k: 1.25 * r for k, r in MEASURED_RATIO.items()}
GATE_CASES = [(n, steps, scale) for n in (4096, 4097, 10000) for steps in (1, 3, 50) for scale in (1e-6, 1e-3, 1.0, 30.0)]


def gate_case(n, steps, scale):
    """(p0, [gradients]) of one gate case, seeded by the case"""
    gen = torch.Generator().manual_seed(n * 1000 + steps)
    p0 = torch.randn(n, generator=gen)
    return p0, [torch.randn(n, generator=gen) * scale for _ in range(steps)]


def offsets(sizes):
    out, off = [], 0
    for n in sizes:
        out.append(off)
        off += n
    return out


def repdepth_like_120():
    """120 chunk sizes shaped like RepDepth's parameter list: a 7x7 stem, 3x3 convolutions with their batch-norm pairs through
    the four widths, 1x1 downsamples, decoder convolutions with biases, and the one-element bias of a disparity head (which
    leaves every later offset odd)"""
    sizes = [64 * 3 * 49, 64, 64]
    for cin, cout, blocks in ((64, 64, 4), (64, 128, 4), (128, 256, 4), (256, 512, 4)):
        for b in range(blocks):
            sizes += [(cin if b == 0 else cout) * cout * 9, cout, cout]
        if cin != cout:
            sizes += [cin * cout, cout, cout]
    for cin, cout in ((512, 256), (512, 256), (256, 128), (256, 128), (128, 64), (128, 64), (64, 32), (96, 32), (32, 16), (16, 16)):
        sizes += [cin * cout * 9, cout]
    sizes += [16 * 9, 1]
    for cin, cout in ((512, 256), (256, 256), (256, 256)):
        sizes += [cin * cout * 9, cout]
    sizes += [256 * 12, 12]
    while len(sizes) < 120:
        sizes += [256, 256]
    return sizes[:120]


def cover(sizes, offs, first, count, blocks, base_residue=0):
    """replay the kernel's decomposition on the host: for the table range [first, first + count) launched with ``blocks``
    workgroups, how often every element of every chunk is touched and by which workgroup its tile is owned -> ([counts per
    chunk as tensors], total tiles).  ``base_residue``: elements by which the flat buffers' base is off the 16-byte grid."""
    touched = [torch.zeros(n, dtype=torch.int32) for n in sizes]
    owners = [set() for _ in range(blocks)]
    r, total_tiles = 0, 0
    plan = []
    for e in range(first, first + count):
        n, off = sizes[e], offs[e]
        if n == 0:
            continue
        head = min((-(off + base_residue)) % 4, n)
        nv = (n - head) // 4
        tiles = max(1, -(-nv // (TILE // 4)))
        plan.append((e, head, nv, tiles, r))
        r = (r + tiles) % blocks
        total_tiles += tiles
    for b in range(blocks):
        for e, head, nv, tiles, r0 in plan:
            n = sizes[e]
            t = b - r0 if b >= r0 else b + (blocks - r0)
            while t < tiles:
                owners[b].add((e, t))
                if t == 0:
                    for tid in range(n - 4 * nv):
                        touched[e][tid if tid < head else head + 4 * nv + (tid - head)] += 1
                lo, hi = t * (TILE // 4), min((t + 1) * (TILE // 4), nv)
                if hi > lo:
                    touched[e][head + 4 * lo:head + 4 * hi] += 1
                t += blocks
    return touched, total_tiles, owners
