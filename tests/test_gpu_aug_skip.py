"""The --temporal step's forked passes skip the augmented samples ("student_overlap" 2, the default).

A sample whose weight 1 - augmentation_mask is an exact 0.0f contributes exact zeros to everything the ensemble pass and the
student's marching pass leave for the loss, so the merged launch (march_pair_kernel) runs only the other samples' tasks,
zero-fills what the dead tasks would have written, and the epilogue forms only the consistency term for them.  The result
must EQUAL "student_overlap" 1 (a launch each, every sample computed) under == -- not a tolerance: only the sign of an exact
zero may differ -- with the step workspace filled with NaN beforehand, so that any read of a map a skipped task never wrote
shows.  Shapes: B=2 at 32x64 (the golden fixture's: 2 strips x 4 segments) and B=5 at 40x128 (3 strips x 5 segments: an odd
segment count, so the bottom-up walk of odd segments, the boundary-row hand-over and a partial last strip are in play); the
compaction does not depend on the image size, it can go wrong at mixed patterns, at segment boundaries and at the first /
last sample.
"""
import ctypes

import numpy as np
import pytest
import torch

from mal_amd.synthetic import make_batch, to_dicts
from tests import golden_io as G
from tests import hip_harness as HH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(2, 32, 64), (5, 40, 128)]
PATTERNS = {"none": lambda B: [0] * B, "all": lambda B: [1] * B, "first": lambda B: [1] + [0] * (B - 1),
            "last": lambda B: [0] * (B - 1) + [1], "alternating": lambda B: [(i + 1) % 2 for i in range(B)]}
SEED = 0x4d414c5eed + 99


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


@pytest.fixture(autouse=True)
def _restore():
    """the two options and the noise source as they were, failures included"""
    from mal_amd import config
    saved = {k: _get(k) for k in ("student_overlap", "side_order")}
    noise = config.noise_source, config.noise_seed
    config.noise_source, config.noise_seed = "philox", SEED
    try:
        yield
    finally:
        config.noise_source, config.noise_seed = noise
        for k, v in saved.items():
            _lib().mal_set_option(k.encode(), v)


def _set(**kw):
    for k, v in kw.items():
        assert _lib().mal_set_option(k.encode(), int(v)) == 0, (k, v)


_BATCHES = {}


def _batch(B, H, W):
    if (B, H, W) not in _BATCHES:
        b = make_batch(B, H, W, seed=311 + B, with_syn=True)
        b["disp_ens"] = (0.5 * (b["disp_teacher"] + b["disp_student"]) * 1.03).clone()  # read by --learn_ens only
        _BATCHES[(B, H, W)] = b
    return _BATCHES[(B, H, W)]


class Runner:
    """one step (forward + backward) of the one-call API on a batch whose augmentation tensor can be rewritten in place"""

    def __init__(self, b, kw, want_maps=False, want_decisions=False):
        from mal_amd import trainer
        self.B, _, self.H, self.W = b["color0"].shape
        self.dev = torch.device(DEV)
        b = dict(b)
        if not kw.get("learn_ens"):
            b.pop("disp_ens", None)
        self.opt = trainer.default_options(height=self.H, width=self.W, batch_size=self.B, **kw)
        self.inputs, self.mono_outputs, self.outputs, self.leaves = to_dicts(b, lambda a, t, inv: None, device=self.dev)
        for f, s in ((-1, "m1"), (1, "p1")):
            self.mono_outputs[("axisangle", 0, f)] = self.leaves["axisangle_" + s]
            self.mono_outputs[("translation", 0, f)] = self.leaves["translation_" + s]
        self.aug = self.outputs["augmentation_mask"]
        assert self.aug.dtype == torch.float32 and self.aug.is_contiguous()  # handed to the library as it is
        self.synth = HH.producer_of(b, self.dev)
        self.one = torch.ones((), device=self.dev)
        self.want = dict(want_maps=want_maps, want_decisions=want_decisions)
        self.hold = {}

    def set_pattern(self, pattern):
        self.aug.copy_(torch.tensor(pattern, dtype=torch.float32).reshape(self.aug.shape))

    def poison(self):
        """NaN over the step workspace of the current stream; the in-kernel noise stream back to its first step"""
        from mal_amd import step
        step._workspace(self.dev, self.B, self.H, self.W).view(torch.float32).fill_(float("nan"))
        step.noise_counter(self.dev).zero_()

    def step(self):
        from mal_amd import step
        for t in self.leaves.values():
            t.grad = None
        losses, _, maps = step.loss_step(self.opt, self.inputs, dict(self.mono_outputs), dict(self.outputs), w_list=[0.7, 0.3],
                                         image_synthesis=self.synth, **self.want)
        losses["loss"].backward(gradient=self.one)
        self.hold = {"losses": {k: v.detach() for k, v in losses.items()}, "maps": maps}

    def result(self):
        torch.cuda.synchronize()
        return ({k: float(v) for k, v in self.hold["losses"].items()},
                {k: t.grad.detach().cpu().clone() for k, t in self.leaves.items() if t.grad is not None},
                {k: v.detach().cpu().clone() for k, v in self.hold["maps"].items()})


def _run(r, overlap, pattern, side_order=0):
    _set(student_overlap=overlap, side_order=side_order)
    r.set_pattern(pattern)
    r.poison()
    r.step()
    return r.result()


def _equal(got, ref, what):
    """== on every loss scalar, leaf gradient and returned map: NaN fails, the sign of an exact zero does not"""
    for k, v in ref[0].items():
        assert got[0][k] == v, (what, k, got[0][k], v)
    assert set(got[1]) == set(ref[1]) and set(got[2]) == set(ref[2])
    for i in (1, 2):
        for k, v in ref[i].items():
            same = got[i][k] == v
            assert bool(same.all()), (what, k, "unequal elements:", int((~same).sum()), "of", same.numel())


@pytest.mark.parametrize("no_ens", [False, True], ids=["ens", "no_ens"])
@pytest.mark.parametrize("B,H,W", SHAPES, ids=["b2_32x64", "b5_40x128"])
def test_skip_equals_no_skip(B, H, W, no_ens):
    kw = {"temporal": True, "no_ens": True} if no_ens else {"temporal": True}
    with torch.cuda.stream(torch.cuda.Stream()):
        r = Runner(_batch(B, H, W), kw)
        for name, f in PATTERNS.items():
            ref = _run(r, 1, f(B))
            assert all(np.isfinite(v) for v in ref[0].values()), (name, ref[0])
            _equal(_run(r, 2, f(B)), ref, (name, "side_order 0"))
            _equal(_run(r, 2, f(B), side_order=1), ref, (name, "side_order 1"))


def test_the_device_decides_at_replay():
    """a graph captured with one pattern, the augmentation tensor rewritten in place to one with another number of dead
    samples, replayed: the eager "student_overlap" 1 step on the new pattern"""
    B, H, W = 5, 40, 128
    s_ = torch.cuda.Stream()
    s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        r = Runner(_batch(B, H, W), {"temporal": True})
        captured, replayed = PATTERNS["alternating"](B), [1, 1, 0, 1, 1]
        assert sum(captured) != sum(replayed)
        ref = _run(r, 1, replayed)
        ref_captured = _run(r, 1, captured)
        _set(student_overlap=2)
        r.set_pattern(captured)
        r.step()  # (eager steps before the capture: the side stream and the workspace exist)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        # captured on THIS stream: the step's workspace is keyed by the stream, and poison() must reach the one the graph uses
        with torch.cuda.graph(graph, stream=s_, capture_error_mode="thread_local"):
            r.step()
        for pattern, want in ((captured, ref_captured), (replayed, ref), ([0] * B, None), (replayed, ref)):
            r.set_pattern(pattern)
            r.poison()
            for t in r.leaves.values():
                t.grad.zero_()
            graph.replay()
            if want is not None:
                _equal(r.result(), want, ("replay", pattern))
    torch.cuda.current_stream().wait_stream(s_)


def check_against_the_oracle(b, kw, n0, n1):
    """a --temporal step on `b` (its augmentation mask as given), no maps requested (the skip applies), against the CPU
    oracle with the gates tests/test_gpu_parity.py::_check_case (test_step_parity) puts on a fixture's scalars and
    gradients; the maps that test reads from the kernels are not returned here, the near-tie sets are the oracle's"""
    B, _, H, W = b["color0"].shape
    assert kw.get("temporal") and not kw.get("main_temporal") and "syn_rects" in b
    o = HH.run_oracle(b, kw, n0, n1)
    from mal_amd import config
    config.noise_source = "given"
    _set(student_overlap=2)
    with torch.cuda.stream(torch.cuda.Stream()):
        r = Runner(b, kw)
        r.poison()
        from mal_amd import step
        losses, _, maps = step.loss_step(r.opt, r.inputs, r.mono_outputs, r.outputs, w_list=[0.7, 0.3], noise=n0.to(DEV),
                                         want_maps=False, image_synthesis=r.synth)
        assert not maps
        losses["loss"].backward()
        torch.cuda.synchronize()
    h = dict(losses={k: float(v.detach()) for k, v in losses.items()},
             grads={k: (t.grad if t.grad is not None else torch.zeros_like(t)).cpu().numpy() for k, t in r.leaves.items()})
    N = B * H * W
    # ---- scalars (the step's names for the oracle's two dictionaries, as tests/test_gpu_step.py::_check_step pairs them)
    amb_distil = HH.near_tie(np.concatenate([m for m in (o["mono_reproj"], o["ens"], o["multi_cands"].min(1, keepdims=True))
                                             if m is not None], 1), 2e-4)
    allow_distil = float((np.abs(o["mono_depth"] - o["multi_depth"]) * amb_distil).sum() / N)
    allow_auto, renorm, any_auto = HH.automask_tie_allowance(o, n0)
    pairs = [(k, v) for k, v in o["losses"].items() if k in h["losses"]]
    pairs += [("mono/loss", o["mono_losses"]["loss"]), ("mono/reproj_loss/0", o["mono_losses"]["reproj_loss/0"])]
    assert {"reproj_loss/0", "consistency_loss/0", "distil_loss", "loss"} <= {k for k, _ in pairs}
    for k, v in pairs:
        tol = 1e-4 * abs(v) + (allow_distil if ("distil" in k or k.startswith("loss")) else 0.0)
        tol += 0.0 if ("distil" in k or "consistency" in k) else allow_auto
        print(k, h["losses"][k], v, tol)
        assert abs(h["losses"][k] - v) <= tol, (k, h["losses"][k], v, tol)
    assert abs(h["losses"]["loss"] - o["final"]) <= 1e-4 * abs(o["final"]) + B * (allow_distil + allow_auto)
    # ---- per-pixel disparity gradients outside the near-tie pixels
    idn = o["ident"] + n0.numpy() * np.float32(1e-5)
    amb_t = HH.dilate3(HH.near_tie(o["mono_cands"], 2e-4, distinct=True) | (np.abs(o["mono_reproj"] - idn) <= 1e-4))
    amb_t |= HH.sample_ambiguous(o["mono_sample"], H, W)
    amb_s = HH.dilate3(HH.near_tie(o["multi_cands"], 2e-4, distinct=True)) | HH.sample_ambiguous(o["multi_sample"], H, W) | amb_distil
    amb_s |= np.abs(o["mono_depth"] - o["multi_depth"]) <= 1e-6 * np.abs(o["mono_depth"])
    amb_t |= HH.dilate3(HH.near_tie(o["mono_cands"], 2e-4, distinct=True))
    for key, amb in (("disp_teacher", amb_t), ("disp_student", amb_s)):
        g, ref = h["grads"][key], o["grads"][key]
        sc = np.abs(ref).max()
        err = np.abs(g - ref)[~amb]
        tol = 2e-4 + (renorm if key == "disp_teacher" else 0.0)
        print(key, err.max() / sc, (err > tol * sc).mean(), amb.mean())
        assert (err > tol * sc).mean() <= 2e-5, (key, err.max() / sc, (err > tol * sc).mean())
        assert amb.mean() <= 0.05, (key, "near-tie fraction", amb.mean())
    # ---- summed gradients: never further from the fp32 reference than it is from fp64
    o64 = HH.oracle_fp64_grads(b, kw, n0, n1)
    l2rel = lambda a, c: float(np.linalg.norm((a - c).ravel()) / (np.linalg.norm(c.ravel()) + 1e-30))
    for key in HH.LEAVES:
        g, ref, r64 = h["grads"][key], o["grads"][key], o64[key]
        if key in ("disp_teacher", "disp_student"):
            keep = ~(amb_t if key == "disp_teacher" else amb_s)
            g, ref, r64 = g[keep], ref[keep], r64[keep]
        floor = l2rel(ref, r64)
        if any_auto and g.ndim != 4 and key != "disp_student":
            continue  # (as _check_case: a pose gradient moves by per cent with the side ONE automask pixel at its threshold takes)
        extra = 0.0 if key == "disp_student" else renorm
        print(key, l2rel(g, ref), floor)
        assert l2rel(g, ref) <= max(1e-4, 1.5 * floor) + extra, (key, l2rel(g, ref), floor)


def test_against_the_oracle():
    """the golden --temporal fixture with the first sample augmented"""
    z = G.load("step_b2_32x64_temporal")
    b = G.batch_from_golden(z)
    B, _, H, W = b["color0"].shape
    b["augmentation_mask"] = torch.tensor([1.0, 0.0]).reshape(b["augmentation_mask"].shape)
    n0, n1 = G.noises(z, (B, 1, H, W))
    check_against_the_oracle(b, G.opt_kwargs(z), n0, n1)


@pytest.mark.parametrize("case", ["want_maps", "decisions", "main_temporal", "dual_distil", "learn_ens"])
def test_the_predicate(case):
    """with maps or decision planes requested, or under --main_temporal / --dual_distil / --learn_ens, every sample is
    computed as under "student_overlap" 1: the returned maps and planes are identical for the augmented samples too"""
    B, H, W = 5, 40, 128
    kw = {"temporal": True}
    want = {}
    if case == "want_maps":
        want = {"want_maps": True}
    elif case == "decisions":
        want = {"want_decisions": True}
    elif case == "main_temporal":
        kw["main_temporal"] = True
    elif case == "dual_distil":
        kw.update(no_ens=True, dual_distil=True)
    else:
        kw["learn_ens"] = True
    pattern = PATTERNS["alternating"](B)
    with torch.cuda.stream(torch.cuda.Stream()):
        r = Runner(_batch(B, H, W), kw, **want)
        ref = _run(r, 1, pattern)
        got = _run(r, 2, pattern)
    if want:
        assert ref[2], "maps were requested"
    for i in (1, 2):  # bit for bit here: the same launches ran
        assert set(got[i]) == set(ref[i])
        for k, v in ref[i].items():
            assert torch.equal(got[i][k], v), (case, k)
    assert got[0] == ref[0]


def test_option_range():
    lib = _lib()
    for v in (0, 1, 2):
        assert lib.mal_set_option(b"student_overlap", v) == 0 and _get("student_overlap") == v
    assert lib.mal_set_option(b"student_overlap", 3) == -1 and lib.mal_set_option(b"student_overlap", -1) == -1
    assert _get("student_overlap") == 2
