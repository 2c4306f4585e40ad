"""What the matcher sweep shares (tests/test_matcher_host.py on the CPU, tests/test_gpu_matcher_sweep.py on the device):
the case table, three mask generators and the gates.

Gates (each on every case unless it says otherwise):
  1. count <= min of the sizes; rows distinct and in range; int64, contiguous, on the device (as tests/test_gpu_matcher.py).
  2. |C - costs_fp64| <= half the fp32 spacing at |D|, plus 1e-12: the kernel forms the cost in fp64 and rounds it ONCE to
     fp32 (the 2.5e-7 of tests/test_gpu_matcher.py is this bound at |D| < 2, here for any weights).
  3. the pairs equal ``R.match(C1, C2)`` on the kernel's OWN returned matrices: mal_match.hip fixes the algorithm (Crouse's
     shortest augmenting paths), the fp64 operation order and "lowest index on a tie", and tests/matcher_restated.py
     states the same, so ties are decided alike.
  4. cases marked ``unique``: the pairs also equal ``R.match(D1, D2)``; the CPU test shows margin >= 1e-4 on both.
  5. bit-identical results across mask kinds and across two runs."""
import functools
import zlib

import numpy as np

from tests import matcher_restated as R

MASK_BYTES = (1, 2, 0x40, 0x80, 0xff)
KINDS = ("bool", "uint8", "float32")
MARGIN = 1e-4


def random_masks(rng, n, H, W, extremes):
    """per-instance densities from sparse to dense; ``extremes``: an empty and a full mask among them"""
    dens = rng.uniform(0.02, 0.9, n)
    m = rng.random((n, H, W)) < dens[:, None, None]
    if extremes and n >= 2:
        m[n // 2] = False
        m[n - 1] = True
    return m


def proto_masks(rng, protos, n, flip):
    """noisy copies of a few prototypes: many near-equal costs, long augmenting paths"""
    pick = rng.integers(0, len(protos), n)
    return protos[pick] ^ (rng.random((n,) + protos.shape[1:]) < flip)


def _ellipse(rng, H, W):
    return [int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(1, max(H // 4, 2) + 1)), int(rng.integers(1, max(W // 6, 2) + 1))]


def ellipse_sets(rng, H, W, sizes):
    """the fixtures' inputs: the target ellipses reappear on both sides jittered by <= 2 px, mixed with distractors"""
    n_n, n_m, n_0 = sizes
    tgt = np.array([_ellipse(rng, H, W) for _ in range(n_0)], dtype=np.int64).reshape(-1, 4)
    out = []
    for n in (n_n, n_m):
        keep = rng.permutation(n_0)[:min(n, n_0)]
        ell = tgt[keep].copy()
        ell[:, :2] += rng.integers(-2, 3, (len(keep), 2))
        extra = np.array([_ellipse(rng, H, W) for _ in range(n - len(keep))], dtype=np.int64).reshape(-1, 4)
        ell = np.concatenate([ell, extra])[rng.permutation(n)] if n else ell.reshape(-1, 4)
        out.append(R.ellipse_masks(ell, H, W))
    return out[0], out[1], R.ellipse_masks(tgt, H, W)


def _c(sizes, hw, gen, classes="mixed", weights=(1.0, 1.0, 1.0), kinds=("bool", "uint8", "float32"), unique=False):
    return dict(sizes=sizes, H=hw[0], W=hw[1], gen=gen, classes=classes, weights=weights, kinds=kinds, unique=unique)


U8F, FBU, UFB = ("uint8", "bool", "float32"), ("float32", "bool", "uint8"), ("uint8", "float32", "bool")
CASES = {
    # both sides above 64: a lane owns a row and a column in two registers
    "rand_128x128x128_96x96_second_pack_trip": _c((128, 128, 128), (96, 96), "rand"),
    "proto_128x128x128_24x40_near_ties": _c((128, 128, 128), (24, 40), "proto", classes="equal", kinds=U8F),
    "rand_128x128x128_50x173_dice_weight_zero": _c((128, 128, 128), (50, 173), "rand", classes="high", weights=(1.0, 1.0, 0.0), kinds=FBU),
    "proto_70x100x128_96x96_class_weight_zero": _c((70, 100, 128), (96, 96), "proto", weights=(0.0, 1.0, 1.0), kinds=UFB),
    "rand_70x100x128_5x13": _c((70, 100, 128), (5, 13), "rand", classes="distinct"),
    "ellipse_128x128x128_24x40": _c((128, 128, 128), (24, 40), "ellipse", kinds=UFB),
    # around 64
    "rand_65x64x63_8x8": _c((65, 64, 63), (8, 8), "rand", kinds=U8F),
    "ellipse_63x65x64_50x173_ten_bit_tail": _c((63, 65, 64), (50, 173), "ellipse", kinds=FBU),
    "rand_63x65x64_3x21_class_weight_zero": _c((63, 65, 64), (3, 21), "rand", classes="distinct", weights=(0.0, 1.0, 1.0)),
    "rand_64x64x64_1x1": _c((64, 64, 64), (1, 1), "rand", classes="equal", kinds=UFB),
    "proto_64x64x64_8x8_high_classes_dice_weight_zero": _c((64, 64, 64), (8, 8), "proto", classes="high", weights=(1.0, 1.0, 0.0)),
    "proto_65x64x63_24x40": _c((65, 64, 63), (24, 40), "proto", classes="high", kinds=FBU),
    # one side of one, very rectangular
    "rand_127x128x1_5x13": _c((127, 128, 1), (5, 13), "rand", kinds=U8F),
    "rand_127x128x1_96x96": _c((127, 128, 1), (96, 96), "rand", classes="equal"),
    "proto_1x128x128_3x21": _c((1, 128, 128), (3, 21), "proto", classes="distinct", kinds=FBU),
    "ellipse_1x128x128_50x173": _c((1, 128, 128), (50, 173), "ellipse"),
    "ellipse_128x3x5_24x40": _c((128, 3, 5), (24, 40), "ellipse", unique=True, kinds=U8F),
    "ellipse_3x5x128_24x40": _c((3, 5, 128), (24, 40), "ellipse", unique=True, kinds=UFB),
    "ellipse_20x24x8_24x40": _c((20, 24, 8), (24, 40), "ellipse", unique=True),
    "rand_20x24x16_24x40": _c((20, 24, 16), (24, 40), "rand", unique=True, kinds=FBU),
    "rand_40x36x12_24x40": _c((40, 36, 12), (24, 40), "rand", unique=True),
    "rand_128x3x5_8x8": _c((128, 3, 5), (8, 8), "rand", classes="high"),
    "rand_3x5x128_1x1": _c((3, 5, 128), (1, 1), "rand"),
    # each side empty in turn
    "empty_n_0x5x4_5x13": _c((0, 5, 4), (5, 13), "rand"),
    "empty_m_5x0x4_5x13": _c((5, 0, 4), (5, 13), "rand", kinds=U8F),
    "empty_0_5x4x0_5x13": _c((5, 4, 0), (5, 13), "rand", kinds=FBU),
}


def _classes(rng, mode, sizes):
    if mode == "equal":
        return [np.full(n, 3, dtype=np.int64) for n in sizes]
    if mode == "distinct":  # no two instances of the three sets share a class
        perm = rng.permutation(sum(sizes)).astype(np.int64)
        return [perm[sum(sizes[:k]):sum(sizes[:k + 1])] for k in range(3)]
    if mode == "high":      # equal in the low 32 bits, different above
        return [np.int64(7) + (rng.integers(0, 3, n).astype(np.int64) << 33) for n in sizes]
    return [rng.integers(0, 5, n).astype(np.int64) for n in sizes]


@functools.lru_cache(maxsize=None)
def make(name):
    """-> dict: the spec, masks_n/m/0 (bool numpy), class_n/m/0 (int64), bytes_n/m/0 (the non-zero byte per set pixel for the
    uint8 kind).  Seeded from the name; a ``unique`` case takes the first seed whose two optima have margin >= 1e-4."""
    spec = CASES[name]
    H, W, sizes = spec["H"], spec["W"], spec["sizes"]
    for attempt in range(40 if spec["unique"] else 1):
        rng = np.random.default_rng([zlib.crc32(name.encode()), attempt])
        if spec["gen"] == "rand":
            masks = [random_masks(rng, n, H, W, extremes=True) for n in sizes]
        elif spec["gen"] == "proto":
            protos = rng.random((4, H, W)) < 0.5
            masks = [proto_masks(rng, protos, n, 0.02) for n in sizes]
        else:
            masks = list(ellipse_sets(rng, H, W, sizes))
        classes = _classes(rng, spec["classes"], sizes)
        d = dict(spec)
        d["name"] = name
        for s, m, c in zip(("n", "m", "0"), masks, classes):
            d["masks_" + s], d["class_" + s] = m, c
            d["bytes_" + s] = rng.choice(np.array(MASK_BYTES, dtype=np.uint8), size=m.shape)
        if not spec["unique"]:
            return d
        D1, D2 = costs(d)
        if min(R.margin_of(D1), R.margin_of(D2)) >= MARGIN:
            return d
    raise AssertionError("case %s: no inputs with a unique optimum found" % name)


def costs(d):
    """the two matrices in fp64 (tests/matcher_restated.costs_fp64) with the case's weights"""
    w_class, _, w_dice = d["weights"]
    return (R.costs_fp64(d["masks_n"], d["masks_0"], d["class_n"], d["class_0"], w_class, w_dice),
            R.costs_fp64(d["masks_m"], d["masks_0"], d["class_m"], d["class_0"], w_class, w_dice))


@functools.lru_cache(maxsize=None)
def reference(name):
    return costs(make(name))


def cost_bound(D):
    """gate 2: half the fp32 spacing at |D| (the binade of |D|: 2^(floor(log2 |D|) - 23)), plus 1e-12"""
    a = np.abs(np.asarray(D, dtype=np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.where(a > 0, 0.5 * np.exp2(e - 23), 0.0) + 1e-12


def nw(H, W):
    return (H * W + 63) // 64


REQUIRED_SIZES = ((128, 128, 128), (127, 128, 1), (1, 128, 128), (65, 64, 63), (63, 65, 64), (64, 64, 64), (128, 3, 5),
                  (3, 5, 128), (70, 100, 128))
REQUIRED_SHAPES = ((1, 1), (3, 21), (8, 8), (5, 13), (24, 40), (96, 96), (50, 173))
