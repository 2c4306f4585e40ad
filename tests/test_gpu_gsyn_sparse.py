"""The --temporal step keeps the cotangent of the synthesised pair sparse (config.syn_grad_sparse, MAL_STEP_GSYN_SPARSE).

With the library's own producer (mal_amd.dyn_utils.image_synthesis: one BatchSynthesisFn node on the hint's leaves, region map,
in-place region-only backward) the fused sweep's tasks that keep more than two pixels away from the region store a byte of the
workspace's tile map instead of zeros into g_syn, and the teacher's gradient sweep skips those tiles.  Nothing the step returns
may change: the switch on against off under torch.equal, with the cotangent buffers, the tile map and the rest of the
workspace filled with NaN beforehand, so that a read of anything a dead task no longer writes shows.

The producer is driven by stand-in masks (boxes) placed against the tile grid of the fused sweep: 60 columns x 4 rows
("syn_rows") per tile, live when a region pixel lies within two pixels of it.  Shapes: B=2 32x64 (the golden shape), B=3 42x136
(the last task of a strip two rows high, the last strip 16 columns, the producer's non-16-byte path), B=2 40x130 (a width
that is no multiple of 4).
"""
import ctypes

import numpy as np
import pytest
import torch

from mal_amd.synthetic import _Instances, make_batch
from tests.test_gpu_aug_skip import Runner, check_against_the_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(2, 32, 64), (3, 42, 136), (2, 40, 130)]
SEED = 0x4d414c5eed + 131
ROWS, CW = 4, 60  # the fused sweep's tile: "syn_rows" rows x 60 columns


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


def _lib():
    from mal_amd import _lib as L
    return L.load()


def _get(name):
    v = ctypes.c_int()
    assert _lib().mal_get_option(name.encode(), ctypes.byref(v)) == 0
    return v.value


def _set(**kw):
    for k, v in kw.items():
        assert _lib().mal_set_option(k.encode(), int(v)) == 0, (k, v)


@pytest.fixture(autouse=True)
def _restore():
    """the options, the noise source and the poisoning hook as they were, failures included"""
    from mal_amd import config, step
    saved = {k: _get(k) for k in ("syn_rows", "student_overlap", "side_order")}
    noise, sparse = (config.noise_source, config.noise_seed), config.syn_grad_sparse
    config.noise_source, config.noise_seed = "philox", SEED
    _set(syn_rows=ROWS)
    step.POISON_COTANGENTS = True
    try:
        yield
    finally:
        step.POISON_COTANGENTS = False
        config.noise_source, config.noise_seed = noise
        config.syn_grad_sparse = sparse
        for k, v in saved.items():
            _lib().mal_set_option(k.encode(), v)


# ---- stand-in masks: per sample None (no confident instance: a host decision, as the score threshold is) or three
# instances (box in the "last" frame, box in the "next" frame), boxes as (y0, y1, x0, x1), inclusive
def pattern_none(B, H, W):
    return [None] * B


def pattern_edges(B, H, W):
    """in tile rows 0 / 3 / 5 of strip 0: a region that ends exactly ON the strip's last column (59), one column short of it
    and two short -- the neighbouring tile of strip 1 is live, live (distance 2) and dead (distance 3); and downwards: the
    regions end on row 1 (two short of tile row 0's last row: tile row 1 dead), row 14 (one short: tile row 4 live) and
    row 23 (exactly: tile row 6 live).  The "next" boxes lie up and / or to the left, so the "last" ones set those edges."""
    one = [((0, 1, 50, 59), (0, 1, 46, 55)), ((13, 14, 49, 58), (12, 13, 45, 54)), ((22, 23, 48, 57), (22, 23, 45, 54))]
    return [one] * B


def pattern_border(B, H, W):
    """instances on the image border: the first rows / columns, the last ones, the last strip's last columns"""
    one = [((0, 2, 0, 4), (0, 3, 0, 6)), ((H - 3, H - 1, W - 5, W - 1), (H - 2, H - 1, W - 8, W - 2)),
           ((H // 2, H // 2 + 1, W - 2, W - 1), (H // 2, H // 2 + 2, W - 3, W - 1))]
    return [one] * B


def pattern_all(B, H, W):
    """every tile holds region pixels"""
    one = [((0, H - 1, 0, W - 4), (0, H - 1, 3, W - 1)), ((2, 5, 3, 9), (3, 6, 6, 12)), ((H - 6, H - 3, W - 12, W - 7), (H - 7, H - 4, W - 14, W - 9))]
    return [one] * B


def pattern_mixed(B, H, W):
    """a sample with instances next to a sample without"""
    kinds = [pattern_edges(1, H, W)[0], None, pattern_border(1, H, W)[0]]
    return [kinds[b % 3] for b in range(B)]


def pattern_moved(B, H, W):
    """pattern_edges with its boxes somewhere else: tiles that were live are dead and the other way round"""
    one = [((22, 23, 10, 19), (21, 22, 6, 15)), ((9, 10, W - 12, W - 3), (8, 9, W - 14, W - 5)), ((H - 4, H - 3, 30, 39), (H - 5, H - 4, 28, 37))]
    return [one] * B


PATTERNS = {"none": pattern_none, "edges": pattern_edges, "border": pattern_border, "all": pattern_all, "mixed": pattern_mixed}


class Stub:
    """the two external models of dyn_utils.image_synthesis (segmenter, matcher) over box masks held on the device; ``write``
    replaces the boxes in place (a captured step reads the new ones), which samples are confident stays as constructed"""

    def __init__(self, B, H, W, pattern, dev):
        self.B, self.H, self.W, self.dev = B, H, W, dev
        self.confident = [s is not None for s in pattern]
        self.masks = [(torch.zeros(3, H, W, dtype=torch.bool, device=dev), torch.zeros(3, H, W, dtype=torch.bool, device=dev))
                      for _ in range(B)]
        self.empty = torch.zeros(3, H, W, dtype=torch.bool, device=dev)
        self.every = torch.arange(3, device=dev)
        self.next_b = -1
        self.region = np.zeros((B, H, W), bool)
        self.write(pattern)

    def write(self, pattern):
        assert [s is not None for s in pattern] == self.confident
        self.region[:] = False
        for b, inst in enumerate(pattern):
            if inst is None:
                continue
            host = np.zeros((2, 3, self.H, self.W), bool)
            for i, pair in enumerate(inst):
                for f, (y0, y1, x0, x1) in enumerate(pair):
                    assert 0 <= y0 <= y1 < self.H and 0 <= x0 <= x1 < self.W, (pair, self.H, self.W)
                    host[f, i, y0:y1 + 1, x0:x1 + 1] = True
            for f in range(2):
                self.masks[b][f].copy_(torch.from_numpy(host[f]))
            self.region[b] = host.any((0, 1))

    def ins_model(self, images):
        if self.next_b < 0:  # a producer call's first: the target frames, only the scores are read
            self.next_b = 0
            assert images.shape[0] == self.B
            return [{"instances": _Instances(torch.full((3,), 0.9 if c else 0.1), self.empty)} for c in self.confident]
        assert images.shape[0] == 2
        while not self.confident[self.next_b]:  # the (warped last, warped next) pair of the next CONFIDENT sample
            self.next_b += 1
        b = self.next_b
        self.next_b += 1
        scores = torch.full((3,), 0.9)
        return [{"instances": _Instances(scores, self.masks[b][0])}, {"instances": _Instances(scores, self.masks[b][1])}]

    def matcher(self, ins_last, ins_next, cur):
        return self.every, self.every

    def synth(self, wrap=False):
        from mal_amd import dyn_utils

        def run(inputs, outputs, scale):
            if wrap:  # one autograd op behind the leaves: the cotangent would be handed to it as a whole
                outputs = _Times1(outputs, scale)
            self.next_b = -1
            return dyn_utils.image_synthesis(inputs, outputs, scale, 0.5, self.ins_model, self.matcher)
        return run

    def expected_live(self):
        """the fused sweep's rule on the region map: a tile is live when a region pixel lies in rows [y_lo - 2, y_hi + 1] and
        columns [x_lo - 2, x_lo + 61] (the 64 lanes of its strip) -> (B, segs, strips) bytes"""
        segs, strips = (self.H + ROWS - 1) // ROWS, (self.W + CW - 1) // CW
        live = np.zeros((self.B, segs, strips), np.uint8)
        for s in range(segs):
            for t in range(strips):
                y0, y1 = max(s * ROWS - 2, 0), min(s * ROWS + ROWS + 1, self.H - 1)
                x0, x1 = max(t * CW - 2, 0), min(t * CW + 61, self.W - 1)
                live[:, s, t] = self.region[:, y0:y1 + 1, x0:x1 + 1].any((1, 2))
        return live


class _Times1(dict):
    """the producer's view of the outputs dict with ``* 1.0`` on the two warped images it reads; what it writes goes to the
    caller's dict"""

    def __init__(self, outer, scale):
        super().__init__(outer)
        self.outer = outer
        for f in (-1, 1):
            dict.__setitem__(self, ("color", f, scale), outer[("color", f, scale)] * 1.0)

    def __setitem__(self, k, v):
        dict.__setitem__(self, k, v)
        self.outer[k] = v


_BATCHES = {}


def _batch(B, H, W):
    if (B, H, W) not in _BATCHES:
        _BATCHES[(B, H, W)] = make_batch(B, H, W, seed=577 + B + W, with_syn=True)
    return _BATCHES[(B, H, W)]


def _runner(B, H, W, pattern, wrap=False):
    r = Runner(_batch(B, H, W), {"temporal": True})
    r.stub = Stub(B, H, W, pattern, r.dev)
    r.synth = r.stub.synth(wrap)
    return r


def _sparse(on):
    from mal_amd import config
    config.syn_grad_sparse = bool(on)


def _run(r, sparse):
    _sparse(sparse)
    r.poison()
    r.step()
    return r.result()


def _same(got, ref, what):
    """torch.equal on every leaf gradient, == on every loss scalar; NaN anywhere fails"""
    assert set(got[0]) == set(ref[0]) and set(got[1]) == set(ref[1]) and got[1], what
    for k, v in ref[0].items():
        assert np.isfinite(v) and got[0][k] == v, (what, k, got[0][k], v)
    for k, v in ref[1].items():
        assert bool(torch.isfinite(v).all()), (what, k, "reference not finite")
        assert torch.equal(got[1][k], v), (what, k, "unequal elements:", int((got[1][k] != v).sum()), "of", v.numel())


def _tile_live(r):
    """the step's tile map: the last block of its workspace (mal_step.hip, carve_step), [B][segs][strips] bytes"""
    from mal_amd import step
    B, H, W = r.B, r.H, r.W
    need = int(_lib().mal_step_workspace_bytes(B, H, W))
    nb = B * ((W + 59) // 60) * ((H + 7) // 8)
    block = (nb * 4 + 255) & ~255
    segs, strips = (H + ROWS - 1) // ROWS, (W + CW - 1) // CW
    torch.cuda.synchronize()
    ws = step._workspace(r.dev, B, H, W)
    return ws[need - block:need - block + B * segs * strips].cpu().numpy().reshape(B, segs, strips)


@pytest.mark.parametrize("B,H,W", SHAPES, ids=["b2_32x64", "b3_42x136", "b2_40x130"])
def test_sparse_equals_dense(B, H, W):
    with torch.cuda.stream(torch.cuda.Stream()):
        for name, f in PATTERNS.items():
            r = _runner(B, H, W, f(B, H, W))
            ref = _run(r, 0)
            got = _run(r, 1)
            _same(got, ref, (name, B, H, W))
            live = _tile_live(r)
            want = r.stub.expected_live()
            assert (live == want).all(), (name, "tile map", live.tolist(), want.tolist())
            if name == "edges":  # both sides of the "within two pixels" rule, sideways and downwards
                assert want[0, 0, 1] == 1 and want[0, 3, 1] == 1 and want[0, 5, 1] == 0, want[0].tolist()
                assert want[0, 1, 0] == 0 and want[0, 4, 0] == 1 and want[0, 6, 0] == 1, want[0].tolist()
            if name == "all":
                assert want.all()
            if name in ("none", "mixed"):
                assert not want[1].any() and (name == "none") == (not want[0].any())


def test_replay_with_rewritten_masks():
    """one captured graph, the masks rewritten in place between replays -- tiles go live -> dead and dead -> live --, against
    the eager dense step on each mask set"""
    B, H, W = 3, 42, 136
    sets = [pattern_edges(B, H, W), pattern_moved(B, H, W), pattern_border(B, H, W), pattern_edges(B, H, W)]
    s_ = torch.cuda.Stream()
    s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        r = _runner(B, H, W, sets[0])
        refs, lives = [], []
        for p in sets[:3]:
            r.stub.write(p)
            refs.append(_run(r, 0))
            lives.append(r.stub.expected_live())
        refs.append(refs[0]), lives.append(lives[0])
        flips = lives[0].astype(int) - lives[1].astype(int)
        assert (flips == 1).any() and (flips == -1).any()  # live -> dead and dead -> live for the same tiles
        _sparse(1)
        r.stub.write(sets[0])
        r.step()  # (eager steps before the capture: the side stream and the workspace exist)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s_, capture_error_mode="thread_local"):
            r.step()
        for p, want, live in zip(sets, refs, lives):
            r.stub.write(p)
            r.poison()
            for t in r.leaves.values():
                t.grad.zero_()
            graph.replay()
            _same(r.result(), want, ("replay", p[0]))
            assert (_tile_live(r) == live).all()
    torch.cuda.current_stream().wait_stream(s_)


def test_an_op_behind_the_leaves_takes_the_dense_path():
    """a producer that wraps dyn_utils.image_synthesis and puts ``* 1.0`` behind the leaves: its backward is handed the
    cotangent as a whole, so the flag stays off, the fused sweep zero-fills, and the switch changes nothing"""
    from mal_amd import _lib as L
    from mal_amd import step
    B, H, W = 2, 40, 130
    seen = []
    keep = step._Hint.finish

    def spy(self, *a, **k):
        keep(self, *a, **k)
        seen.append((self.gsyn_sparse, bool(self.a.flags & L.STEP_GSYN_SPARSE)))

    step._Hint.finish = spy
    try:
        with torch.cuda.stream(torch.cuda.Stream()):
            r = _runner(B, H, W, pattern_edges(B, H, W), wrap=True)
            ref = _run(r, 0)
            got = _run(r, 1)
            assert seen == [(False, False)] * 2, seen
            _same(got, ref, "wrapped")
            plain = _runner(B, H, W, pattern_edges(B, H, W))
            del seen[:]
            # (not held against `ref` bit for bit: the wrapped producer's backward cannot ride on the library's side stream, and
            # the teacher's sweep then finishes its gradient itself instead of the assembly -- another rounding of the same sum)
            _run(plain, 1)
            assert seen == [(True, True)], seen  # ... while the producer itself on the leaves gets the flag
    finally:
        step._Hint.finish = keep


def test_against_the_oracle_b12():
    """B=12 at 24x122 with the headline's producer (three elliptic instances per sample), the sparse cotangent on, against
    the CPU oracle under the gates of tests/test_gpu_aug_skip.py::test_against_the_oracle"""
    B, H, W = 12, 24, 122
    b = make_batch(B, H, W, seed=913, with_syn=True)
    b["syn_instances"] = (3, 1234)
    g = torch.Generator().manual_seed(17)
    n0, n1 = torch.randn(B, 1, H, W, generator=g), torch.randn(B, 1, H, W, generator=g)
    _sparse(1)
    check_against_the_oracle(b, {"temporal": True}, n0, n1)


def test_the_switch_off_keeps_the_flag_off():
    """config.syn_grad_sparse = False: the producer on the leaves gets the dense zero-fill -- the tile map is never written"""
    B, H, W = 2, 32, 64
    with torch.cuda.stream(torch.cuda.Stream()):
        r = _runner(B, H, W, pattern_edges(B, H, W))
        _sparse(0)
        r.poison()
        before = _tile_live(r).copy()
        r.step()
        assert (_tile_live(r) == before).all()  # still the poison
        _run(r, 1)
        assert (_tile_live(r) == r.stub.expected_live()).all()
