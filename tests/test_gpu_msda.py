"""GPU: mal_amd.msda (mal_msda_fwd / mal_msda_fused_fwd, one HIP launch each) against the reference's own outputs
(tests/golden/msda_*.npz, written by scripts/gen_golden_msda.py) and the checker tests/msda_restated.py evaluated in fp64
on the host.  No test here reads the reference tree.

Gates.  || hip - ref64 ||_2 / || ref64 ||_2 <= max(1.25 x ref_dist, 1e-6), where ref_dist is the same distance of the
reference's own fp32 evaluation (stored in the fixture; for the sweep, of the checker evaluated in fp32): the project's
clause for two fp32 roundings of one function, with its floor.  Case x is exact in fp32 in any order of operations
(locations on a 1/128 grid, weights multiples of 1/64, integer values) and must be EQUAL bit for bit.  The two routes of
the module are two fp32 evaluations, each inside the gate, and are held to twice the gate against each other.  Measured
distances: DESIGN.md 13."""
import functools
import sys

import numpy as np
import pytest
import torch

from mal_amd import msda
from tests import msda_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@functools.lru_cache(maxsize=None)
def case(tag):
    return R.load_case(tag)


def run(value, shapes, start, loc, weights):
    out = msda.ms_deform_attn(dev(value), shapes, start, dev(loc), dev(weights))
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous()
    assert tuple(out.shape) == (value.shape[0], loc.shape[1], value.shape[2] * value.shape[3])
    return out.cpu().numpy()


@pytest.mark.parametrize("tag", list(R.CASES))
def test_fixture_cases(tag):
    d = case(tag)
    args = (d["value"], d["shapes"], d["start"], d["loc"], d["weights"])
    out, again = run(*args), run(*args)
    assert np.array_equal(bits(out), bits(again))  # no atomics, one order
    dist = R.rel_dist(out, d["ref64"])
    print("case %s: kernel distance from fp64 %.3g (reference's %.3g, gate %.3g)" % (tag, dist, d["ref_dist"], R.gate(d["ref_dist"])))
    if tag == "x":
        assert np.array_equal(bits(out), bits(d["ref64"].astype(np.float32)))
    assert dist <= R.gate(d["ref_dist"])
    # the level table as int64 device tensors (upstream's calling convention) is the same call
    dv = msda.ms_deform_attn(dev(d["value"]), dev(np.array(d["shapes"], np.int64)), dev(np.array(d["start"], np.int64)),
                             dev(d["loc"]), dev(d["weights"])).cpu().numpy()
    assert np.array_equal(bits(dv), bits(out))


def load_module(d, fused):
    m = msda.MSDeformAttn(**R.MODULE_CFG, fused=fused)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in d["sd"].items()}, strict=True)
    return m.to(DEV).eval().requires_grad_(False)


@pytest.mark.parametrize("tag", list(R.MODULE_CASES))
def test_module_fixtures(tag):
    d = case(tag)
    mask = None if d["mask"] is None else dev(d["mask"])
    outs = {}
    for fused in (True, False):
        m = load_module(d, fused)
        with torch.no_grad():
            o = m(dev(d["query"]), dev(d["ref"]), dev(d["inp"]), d["shapes"], d["start"], mask)
        assert tuple(o.shape) == d["out64"].shape and o.dtype == torch.float32
        outs[fused] = o.cpu().numpy()
        dist = R.rel_dist(outs[fused], d["out64"])
        print("case %s fused=%s: distance from the module's fp64 output %.3g (reference's %.3g, gate %.3g)"
              % (tag, fused, dist, d["ref_dist"], R.gate(d["ref_dist"])))
        assert dist <= R.gate(d["ref_dist"])
    between = R.rel_dist(outs[True], outs[False])
    print("case %s: fused against unfused %.3g" % (tag, between))
    assert between <= 2 * R.gate(d["ref_dist"])
    # the fused entry on the fixture's own offsets and logits against the checker's operator in fp64
    N, Lq = d["query"].shape[:2]
    M, L, P = R.MODULE_CFG["n_heads"], R.MODULE_CFG["n_levels"], R.MODULE_CFG["n_points"]
    value = np.random.default_rng(5).standard_normal((N, d["inp"].shape[1], M, 16)).astype(np.float32)
    off, lg = d["offsets"].reshape(N, Lq, M, L, P, 2), d["logits"].reshape(N, Lq, M, L * P)
    got = msda.ms_deform_attn_fused(dev(value), d["shapes"], d["start"], dev(off), dev(lg), dev(d["ref"])).cpu().numpy()
    ref = {}
    for t in (np.float64, np.float32):
        ref[t] = R.core(value, d["shapes"], d["start"], R.locations(off, d["ref"], d["shapes"], t),
                        R.softmax(lg, t).reshape(N, Lq, M, L, P), t)
    assert R.rel_dist(got, ref[np.float64]) <= R.gate(R.rel_dist(ref[np.float32], ref[np.float64]))


def test_module_refuses_a_gradient():
    d = case("m4")
    m = load_module(d, True)
    q = dev(d["query"]).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="dyn_utils.py:185-186"):
        m(q, dev(d["ref"]), dev(d["inp"]), d["shapes"], d["start"])
    with torch.no_grad():
        assert not m(q, dev(d["ref"]), dev(d["inp"]), d["shapes"], d["start"]).requires_grad


@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("L", [1, 3, 4])
@pytest.mark.parametrize("M,D", [(8, 32), (1, 4), (3, 5), (2, 64)])
def test_sweep_against_the_checker(M, D, L, P):
    worst = 0.0
    for N in (1, 3):
        for Lq in (1, 63, 64, 65, 257):
            value, levels, start, loc, w = R.sweep_inputs(1000 * N + Lq, N, Lq, M, D, L, P)
            assert (1, 1) in levels or L == 1
            out = run(value, levels, start, loc, w)
            c64, c32 = R.core(value, levels, start, loc, w, np.float64), R.core(value, levels, start, loc, w, np.float32)
            dist, own = R.rel_dist(out, c64), R.rel_dist(c32, c64)
            worst = max(worst, dist)
            assert dist <= R.gate(own), (N, Lq, dist, own)
    print("M=%d D=%d L=%d P=%d: largest kernel distance from the fp64 checker %.3g" % (M, D, L, P, worst))


def test_strided_inputs_equal_their_contiguous_copies():
    value, levels, start, loc, w = R.sweep_inputs(11, 2, 65, 3, 8, 3, 4)
    ref = run(value, levels, start, loc, w)
    v2 = dev(np.stack([value, -value], -1))[..., 0]            # every fourth byte pair skipped: stride 2 in D
    l2 = dev(np.ascontiguousarray(loc.transpose(1, 0, 2, 3, 4, 5))).transpose(0, 1)
    w2 = dev(np.concatenate([w, w], -1))[..., :w.shape[-1]]
    assert not v2.is_contiguous() and not l2.is_contiguous() and not w2.is_contiguous()
    out = msda.ms_deform_attn(v2, levels, start, l2, w2).cpu().numpy()
    assert np.array_equal(bits(out), bits(ref))
    # D % 4 == 0 on a base address that is not 16-byte aligned: the one-channel path, the same numbers
    flat = torch.zeros(value.size + 1, dtype=torch.float32, device=DEV)
    v3 = flat[1:].view(value.shape)
    v3.copy_(dev(value))
    assert v3.is_contiguous() and v3.data_ptr() % 16 == 4
    out = msda.ms_deform_attn(v3, levels, start, dev(loc), dev(w)).cpu().numpy()
    assert np.array_equal(bits(out), bits(ref))


def test_a_side_stream_is_followed():
    value, levels, start, loc, w = R.sweep_inputs(12, 3, 257, 8, 32, 3, 4)
    ref = run(value, levels, start, loc, w)
    v, l, wt = dev(value), dev(loc), dev(w)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x = torch.ones(1 << 25, device=DEV)
        for _ in range(16):  # work in front of the call on this stream: value is final only when it is done
            x = x * 1.0
        late = v * x[0]
        out = msda.ms_deform_attn(late, levels, start, l, wt)
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(bits(out.cpu().numpy()), bits(ref))


def test_graph_capture_and_replay():
    value, levels, start, loc, w = R.sweep_inputs(13, 2, 65, 8, 32, 3, 4)
    v, l, wt = dev(value), dev(loc), dev(w)
    shp, st = dev(np.array(levels, np.int64)), dev(np.array(start, np.int64))
    eager = msda.ms_deform_attn(v, shp, st, l, wt).cpu().numpy()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        out = msda.ms_deform_attn(v, shp, st, l, wt)
    v.mul_(2.0)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(2.0 * eager))  # doubling is exact


def test_nonfinite_locations_contribute_zero():
    value, levels, start, loc, w = R.sweep_inputs(14, 1, 64, 2, 8, 3, 4)
    loc = loc.copy()
    flat = loc.reshape(-1, 2)
    for k, bad in enumerate((np.nan, np.inf, -np.inf, 3e38, -3e38)):
        flat[7 * k::31, k % 2] = bad
    out = run(value, levels, start, loc, w)
    assert np.isfinite(out).all()
    w0 = np.where(np.isfinite(loc).all(-1) & (np.abs(loc) < 1e38).all(-1), w, 0).astype(np.float32)
    clean = np.where(np.isfinite(loc) & (np.abs(loc) < 1e38), loc, 0.5).astype(np.float32)
    assert np.array_equal(bits(out), bits(run(value, levels, start, clean, w0)))


def test_a_level_outside_value_contributes_zero():
    """the device-side guard: start + H W beyond S, or a negative start, switches the level off.  value is the middle of a
    larger buffer here, so that the rows such a table points at exist."""
    value, levels, start, loc, w = R.sweep_inputs(15, 1, 65, 2, 8, 3, 4)
    room = torch.zeros((3,) + value.shape[1:], dtype=torch.float32, device=DEV)
    room[1].copy_(dev(value[0]))
    v, l = room[1:2], dev(loc)
    shp = dev(np.array(levels, np.int64))
    for lvl, wrong in ((2, start[2] + 1), (0, -1), (1, 1 << 40)):
        st = list(start)
        st[lvl] = wrong
        out = msda.ms_deform_attn(v, shp, dev(np.array(st, np.int64)), l, dev(w)).cpu().numpy()
        w0 = w.copy()
        w0[:, :, :, lvl] = 0
        assert np.array_equal(bits(out), bits(run(value, levels, start, loc, w0))), (lvl, wrong)
    big = np.array(levels, np.int64)
    big[0] = (1 << 33, 1 << 33)  # H W overflows 64 bits unless H and W are tested first
    out = msda.ms_deform_attn(v, dev(big), dev(np.array(start, np.int64)), l, dev(w)).cpu().numpy()
    w0 = w.copy()
    w0[:, :, :, 0] = 0
    assert np.array_equal(bits(out), bits(run(value, levels, start, loc, w0)))


def test_other_dtypes_and_shapes_are_refused():
    from mal_amd._lib import MalError
    d = case("d")
    v, l, w = dev(d["value"]), dev(d["loc"]), dev(d["weights"])
    for bad in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(MalError, match=str(bad)):
            msda.ms_deform_attn(v.to(bad), d["shapes"], d["start"], l, w)
    with pytest.raises(MalError, match="level_start_index"):  # the host-side check of a host table
        msda.ms_deform_attn(v, d["shapes"], [1], l, w)
    with pytest.raises(MalError, match="unsupported shape"):  # D = 65: the entry point's own bound
        msda.ms_deform_attn(torch.zeros(1, 12, 1, 65, device=DEV), d["shapes"], d["start"], l[:1], w[:1])


def test_the_drop_in_extension(monkeypatch):
    monkeypatch.delitem(sys.modules, msda.EXTENSION_NAME, raising=False)
    msda.install_extension()
    import MultiScaleDeformableAttention as ext
    d = case("c")
    v, l, w = dev(d["value"]), dev(d["loc"]), dev(d["weights"])
    shp, st = dev(np.array(d["shapes"], np.int64)), dev(np.array(d["start"], np.int64))
    a = ext.ms_deform_attn_forward(v, shp, st, l, w, 128)
    b = msda.ms_deform_attn(v, shp, st, l, w)
    assert torch.equal(a, b)
    with pytest.raises(NotImplementedError, match="trainer.py:354"):
        ext.ms_deform_attn_backward(v, shp, st, l, w, a, 128)
