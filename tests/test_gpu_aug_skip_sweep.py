"""The augmented-sample skip ("student_overlap" 2: march_pair_kernel, the dead-sample branch of step_epilogue_block) swept over
the table of tests/aug_skip_checks.py: batch sizes 1 .. 65 (sample numbers at and past 32, B = 64, the fallback at 65), one
task per sample, decompositions where the two sub-passes differ, a one-row last segment, live task counts on both sides of a
multiple of 8, the scalar branch of the dead epilogue, weights that are neither 0 nor 1, and the weight formed on the host.

The gate is the one of tests/test_gpu_aug_skip.py: a step under "student_overlap" 2 EQUALS the step under 1 (a launch per
pass, every sample computed) under == in every loss scalar and leaf gradient -- NaN fails, only the sign of an exact zero may
differ -- with the step workspace filled with NaN beforehand.  The last test holds the pair of launches to the CPU oracle at
the headline's batch size."""
import numpy as np
import pytest
import torch

from mal_amd.synthetic import make_batch
from tests import aug_skip_checks as A
from tests.test_gpu_aug_skip import SEED, Runner, _batch, _equal, _get, _lib, _run, _set, check_against_the_oracle

pytestmark = pytest.mark.gpu
OPTIONS = ("student_overlap", "side_order", "march_rows", "march_rows_fwd")
TINY = 1.0 - 2.0 ** -24  # the largest float32 below 1: the weight 1 - mask = 2^-24 is tiny and not zero, the sample is live


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


@pytest.fixture(autouse=True)
def _restore():
    """the options and the noise source as they were, failures included"""
    from mal_amd import config
    saved = {k: _get(k) for k in OPTIONS}
    noise = config.noise_source, config.noise_seed
    config.noise_source, config.noise_seed = "philox", SEED
    try:
        yield
    finally:
        config.noise_source, config.noise_seed = noise
        for k, v in saved.items():
            _lib().mal_set_option(k.encode(), v)


def _rows(c):
    _set(march_rows=c.rows, march_rows_fwd=c.rows)


def _finite(ref, what):
    assert all(np.isfinite(v) for v in ref[0].values()), (what, ref[0])


@pytest.mark.parametrize("c", A.CASES, ids=[c.name for c in A.CASES])
def test_skip_equals_no_skip(c):
    _rows(c)
    modes = [({"temporal": True}, (0, 1) if c.extra else (0,))]
    if c.extra:
        modes.append(({"temporal": True, "no_ens": True}, (0, 1)))
    with torch.cuda.stream(torch.cuda.Stream()):
        for kw, orders in modes:
            r = Runner(_batch(c.B, c.H, c.W), kw)
            for name, pattern in A.patterns(c.B).items():
                ref = _run(r, 1, pattern)
                _finite(ref, (name, kw))
                for order in orders:
                    _equal(_run(r, 2, pattern, side_order=order), ref, (c.name, name, kw, "side_order", order))


FRACTIONAL = {
    "quarter_tiny_one": (0.25, 1, 0, TINY, 1, 0.25, 0, 1, TINY, 0, 1, 0.25),
    "all_tiny": (TINY,) * 12,                 # every sample live with the weight 2^-24
    "ones_and_tiny": (1,) * 5 + (TINY,) + (1,) * 6,   # one live sample, numbered 5, among exact ones
    "ones_and_quarter": (1,) * 11 + (0.25,),
    "tiny_first": (TINY,) + (1,) * 11,
}


def test_weights_that_are_not_0_or_1():
    c = A.case("b12_24x122_r8")
    _rows(c)
    for name, pattern in FRACTIONAL.items():
        v = torch.tensor(pattern, dtype=torch.float32)
        assert bool(((1.0 - v) != 0).eq(torch.tensor([p != 1 for p in pattern])).all()), name  # live: all but the exact ones
    with torch.cuda.stream(torch.cuda.Stream()):
        r = Runner(_batch(c.B, c.H, c.W), {"temporal": True})
        for name, pattern in FRACTIONAL.items():
            ref = _run(r, 1, pattern)
            _finite(ref, name)
            for order in (0, 1):
                _equal(_run(r, 2, pattern, side_order=order), ref, (name, "side_order", order))


def _forms(pattern, dev):
    """the mask in the forms loss_step turns into the weight 1 - mask itself ("aug_is_mask" false)"""
    B = len(pattern)
    f32 = torch.tensor(pattern, dtype=torch.float32, device=dev).reshape(B, 1, 1, 1)
    out = {"float64": f32.to(torch.float64)}
    wide = torch.empty(2 * B, 1, 1, 1, dtype=torch.float32, device=dev)
    wide[0::2] = f32
    wide[1::2] = 1.0 - f32  # (what a read of the wrong elements would find)
    out["strided"] = wide[0::2]
    if set(pattern) <= {0, 1}:
        out["bool"] = f32 != 0
    for k, t in out.items():
        assert t.shape == (B, 1, 1, 1) and not (t.dtype == torch.float32 and t.is_contiguous()), k
    return out


def _run_given(r, overlap, aug):
    _set(student_overlap=overlap, side_order=0)
    r.outputs["augmentation_mask"] = aug
    try:
        r.poison()
        r.step()
        return r.result()
    finally:
        r.outputs["augmentation_mask"] = r.aug


@pytest.mark.parametrize("name", ["b12_24x122_r8", "b33_16x24"])
def test_the_weight_formed_on_the_host(name):
    c = A.case(name)
    _rows(c)
    p = A.patterns(c.B)
    todo = [p["alternating"], p["bernoulli_0"], p["bernoulli_1"]]
    if c.B == 12:
        todo += [p["last_live"], p["dead_6"], FRACTIONAL["quarter_tiny_one"]]
    else:  # only the samples numbered 32 and up live, only they dead
        todo += [(1,) * 32 + (0,) * (c.B - 32), (0,) * 32 + (1,) * (c.B - 32)]
    assert all(len(v) == c.B for v in todo)
    with torch.cuda.stream(torch.cuda.Stream()):
        r = Runner(_batch(c.B, c.H, c.W), {"temporal": True})
        for pattern in todo:
            as_mask = _run(r, 2, pattern)
            _finite(as_mask, pattern)
            for form, aug in _forms(pattern, r.dev).items():
                ref = _run_given(r, 1, aug)
                got = _run_given(r, 2, aug)
                _equal(got, ref, (form, pattern, "against student_overlap 1 given the same tensor"))
                _equal(got, as_mask, (form, pattern, "against the contiguous float32 mask"))


def test_replay_at_the_headline_batch_size():
    """one graph captured at B=12 with 6 dead samples, the mask rewritten in place, replayed: each replay is the eager
    "student_overlap" 1 step on its pattern"""
    c = A.case("b12_24x122_r8")
    _rows(c)
    captured = (1,) * 6 + (0,) * 6
    replays = [(1,) * k + (0,) * (12 - k) for k in (0, 1, 6, 11, 12)] + [A.patterns(c.B)["alternating"]]
    s_ = torch.cuda.Stream()
    s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        r = Runner(_batch(c.B, c.H, c.W), {"temporal": True})
        refs = [_run(r, 1, pattern) for pattern in replays]
        _set(student_overlap=2)
        r.set_pattern(captured)
        r.step()  # (eager steps before the capture: the side stream and the workspace exist)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        # captured on THIS stream: the step's workspace is keyed by the stream, and poison() must reach the one the graph uses
        with torch.cuda.graph(graph, stream=s_, capture_error_mode="thread_local"):
            r.step()
        for pattern, want in zip(replays, refs):
            r.set_pattern(pattern)
            r.poison()
            for t in r.leaves.values():
                t.grad.zero_()
            graph.replay()
            _equal(r.result(), want, ("replay", pattern))
    torch.cuda.current_stream().wait_stream(s_)


def test_against_the_oracle_at_the_headline_batch_size():
    """B=12 at 24x122 (3 strips against 2, three segments), samples 0 and 3..8 augmented: near-tie fractions of the oracle on
    this batch 0.019 (teacher) and 0.015 (student)"""
    B, H, W = 12, 24, 122
    b = make_batch(B, H, W, seed=323, with_syn=True)
    b["augmentation_mask"] = torch.tensor([1, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0], dtype=torch.float32).reshape(b["augmentation_mask"].shape)
    torch.manual_seed(1)
    n0, n1 = torch.randn(B, 1, H, W), torch.randn(B, 1, H, W)
    check_against_the_oracle(b, {"temporal": True}, n0, n1)
