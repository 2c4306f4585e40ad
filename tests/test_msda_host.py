"""CPU: the checker of mal_amd.msda (tests/msda_restated.py) against the reference's own outputs
(tests/golden/msda_*.npz, scripts/gen_golden_msda.py); the argument validation of ``mal_msda_fwd`` /
``mal_msda_fused_fwd`` (no device is needed: nothing is launched); the drop-in extension module, the refusals and the
module's state dict.

Gates.  The checker in fp64 must reproduce each fixture's fp64 output to 1e-12 (two fp64 evaluations of one function, a
few dozen operations deep).  The checker in fp32 is what the kernel computes, up to exp's last bit in the fused route; it
must sit inside the GPU tests' gate, max(1.25 x the reference's own fp32 distance, 1e-6), on every fixture: a fixture
that cannot hold that gate with the reference's own arithmetic would be a wrong fixture.  Case x is exact in fp32 in any
order and must come out bit for bit."""
import ctypes
import inspect
import sys

import numpy as np
import pytest
import torch

from mal_amd import msda
from tests import msda_restated as R


@pytest.fixture(scope="module")
def lib():
    from mal_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("tag", list(R.CASES))
def test_checker_reproduces_the_reference(tag):
    d = R.load_case(tag)
    N, M, D, P, levels, Lq = R.CASES[tag]
    start, S = R.starts_of(levels)
    Lq = S if Lq is None else Lq
    assert d["shapes"] == list(levels) and d["start"] == start
    assert d["value"].shape == (N, S, M, D) and d["loc"].shape == (N, Lq, M, len(levels), P, 2)
    assert d["weights"].shape == (N, Lq, M, len(levels), P) and d["ref64"].shape == (N, Lq, M * D)
    assert d["ref32"].dtype == np.float32 and d["ref64"].dtype == np.float64
    assert np.isclose(R.rel_dist(d["ref32"], d["ref64"]), d["ref_dist"], rtol=1e-9, atol=0)
    args = (d["value"], d["shapes"], d["start"], d["loc"], d["weights"])
    c64, c32 = R.core(*args, np.float64), R.core(*args, np.float32)
    d64, d32 = R.rel_dist(c64, d["ref64"]), R.rel_dist(c32, d["ref64"])
    print("case %s: checker fp64 %.3g, checker fp32 %.3g, reference fp32 %.3g, gate %.3g" % (tag, d64, d32, d["ref_dist"], R.gate(d["ref_dist"])))
    assert d64 <= 1e-12
    assert d32 <= R.gate(d["ref_dist"])
    assert d["ref_dist"] < 1e-6


def test_case_x_is_exact():
    d = R.load_case("x")
    assert d["ref_dist"] == 0.0 and np.array_equal(d["ref32"].astype(np.float64), d["ref64"])
    assert np.array_equal(d["loc"] * 128, np.round(d["loc"] * 128)) and (d["loc"] < 0).any() and (d["loc"] > 1).any()
    assert np.array_equal(d["weights"] * 64, np.round(d["weights"] * 64))
    assert np.array_equal(d["weights"].reshape(d["weights"].shape[:3] + (-1,)).sum(-1), np.ones(d["weights"].shape[:3], np.float32))
    assert np.array_equal(d["value"], np.round(d["value"])) and np.abs(d["value"]).max() <= 8
    c32 = R.core(d["value"], d["shapes"], d["start"], d["loc"], d["weights"], np.float32)
    assert c32.dtype == np.float32 and np.array_equal(c32.view(np.int32), d["ref64"].astype(np.float32).view(np.int32))


def test_case_b_holds_the_boundary_samples():
    d = R.load_case("b")
    (H, W), loc = d["shapes"][0], d["loc"].reshape(-1, 2).astype(np.float64)
    x, y = loc[:, 0] * W - 0.5, loc[:, 1] * H - 0.5
    for xv in (-1, 0, W - 1, W):
        for yv in (-1, 0, H - 1, H):
            assert (np.isclose(x, xv, atol=1e-5) & np.isclose(y, yv, atol=1e-5)).any(), (xv, yv)
    assert np.mean((loc < 0).any(1) | (loc > 1).any(1)) > 0.5  # most samples outside the map


@pytest.mark.parametrize("tag", list(R.MODULE_CASES))
def test_checker_reproduces_the_module(tag):
    d = R.load_case(tag)
    assert d["ref"].shape[-1] == R.MODULE_CASES[tag] and (d["mask"] is not None) == (tag == "m2")
    args = (d["sd"], d["query"], d["ref"], d["inp"], d["shapes"], d["start"], d["mask"])
    o64, _, _ = R.module_forward(*args, np.float64)
    o32, off32, lg32 = R.module_forward(*args, np.float32)
    d64, d32 = R.rel_dist(o64, d["out64"]), R.rel_dist(o32, d["out64"])
    print("case %s: checker fp64 %.3g, checker fp32 %.3g, reference fp32 %.3g, gate %.3g" % (tag, d64, d32, d["ref_dist"], R.gate(d["ref_dist"])))
    assert d64 <= 1e-12
    assert d32 <= R.gate(d["ref_dist"])
    assert np.isclose(R.rel_dist(d["out32"], d["out64"]), d["ref_dist"], rtol=1e-9, atol=0)
    # the stored intermediates are the two linear layers' outputs
    assert R.rel_dist(off32.reshape(d["offsets"].shape), d["offsets"]) <= 1e-6
    assert R.rel_dist(lg32.reshape(d["logits"].shape), d["logits"]) <= 1e-6
    assert all(np.abs(v).min() > 0 for v in d["sd"].values())


def test_abi_validation_without_device(lib):
    from mal_amd import _lib as L
    assert lib.mal_msda_fwd(None) == -1 and lib.mal_msda_fused_fwd(None) == -1
    buf = (ctypes.c_float * 4)()  # a host address: validation must end before anything reads it
    ptr = ctypes.addressof(buf)

    def args(**kw):
        a = L.MsdaArgs()
        for n in ("value", "spatial_shapes", "level_start_index", "sampling_locations", "attention_weights",
                  "reference_points", "out"):
            setattr(a, n, ptr)
        a.N, a.S, a.M, a.D, a.L, a.P, a.Lq, a.ref_dim = 1, 4, 1, 4, 1, 1, 1, 2
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    for name in ("value", "spatial_shapes", "level_start_index", "sampling_locations", "attention_weights", "out"):
        assert lib.mal_msda_fwd(args(**{name: None})) == -1, name
        assert lib.mal_msda_fused_fwd(args(**{name: None})) == -1, name
    assert lib.mal_msda_fused_fwd(args(reference_points=None)) == -1
    bad = [dict(L=0), dict(L=9), dict(P=0), dict(P=9), dict(L=5, P=7), dict(D=0), dict(D=65), dict(M=0), dict(N=0),
           dict(S=0), dict(Lq=0), dict(N=1 << 20, S=1 << 20)]
    for kw in bad:
        assert lib.mal_msda_fwd(args(**kw)) == -2, kw
        assert lib.mal_msda_fused_fwd(args(**kw)) == -2, kw
    assert lib.mal_msda_fused_fwd(args(ref_dim=3)) == -2
    assert lib.mal_msda_fwd(args(D=0, value=None)) == -1  # pointers first
    assert b"mal_msda" in lib.mal_strerror(-2)


def test_install_extension(monkeypatch):
    monkeypatch.delitem(sys.modules, msda.EXTENSION_NAME, raising=False)
    mod = msda.install_extension()
    assert msda.install_extension() is mod  # idempotent
    import MultiScaleDeformableAttention as ext
    assert ext is mod
    assert list(inspect.signature(ext.ms_deform_attn_forward).parameters) == [
        "value", "spatial_shapes", "level_start_index", "sampling_loc", "attn_weight", "im2col_step"]
    assert list(inspect.signature(ext.ms_deform_attn_backward).parameters) == [
        "value", "spatial_shapes", "level_start_index", "sampling_loc", "attn_weight", "grad_output", "im2col_step"]
    # a foreign module under that name is not replaced
    import types
    from mal_amd._lib import MalError
    monkeypatch.setitem(sys.modules, msda.EXTENSION_NAME, types.ModuleType(msda.EXTENSION_NAME))
    with pytest.raises(MalError, match="already loaded"):
        msda.install_extension()


def test_backward_refuses_with_the_citation():
    with pytest.raises(NotImplementedError) as e:
        msda.ms_deform_attn_backward(None, None, None, None, None, None, 128)
    assert "dyn_utils.py:185-186" in str(e.value) and "trainer.py:354" in str(e.value)


def test_cpu_tensors_are_refused():
    from mal_amd._lib import MalError
    v, loc, w = torch.zeros(1, 4, 1, 4), torch.zeros(1, 1, 1, 1, 1, 2), torch.ones(1, 1, 1, 1, 1)
    with pytest.raises(MalError, match="device tensor"):
        msda.ms_deform_attn(v, [(2, 2)], [0], loc, w)
    with pytest.raises(MalError, match="device tensor"):
        msda.ms_deform_attn_forward(v, torch.tensor([[2, 2]]), torch.tensor([0]), loc, w, 128)
    m = msda.MSDeformAttn(d_model=8, n_levels=1, n_heads=2, n_points=1)
    with torch.no_grad(), pytest.raises(MalError, match="device tensor"):
        m(torch.zeros(1, 1, 8), torch.zeros(1, 1, 1, 2), torch.zeros(1, 4, 8), [(2, 2)], [0])
    with pytest.raises(NotImplementedError, match="trainer.py:354"):  # grad enabled, parameters require grad
        m(torch.zeros(1, 1, 8), torch.zeros(1, 1, 1, 2), torch.zeros(1, 4, 8), [(2, 2)], [0])


def test_level_table_is_checked_on_the_host():
    from mal_amd._lib import MalError
    hw, st = msda.check_levels([(6, 20), (3, 10), (2, 5)], [0, 120, 150], 160)
    assert hw == ((6, 20), (3, 10), (2, 5)) and st == (0, 120, 150)
    assert msda.check_levels(torch.tensor([[6, 20], [3, 10]]), torch.tensor([0, 120]), 150)[1] == (0, 120)
    with pytest.raises(MalError, match="level_start_index"):
        msda.check_levels([(6, 20), (3, 10), (2, 5)], [0, 120, 151], 160)
    with pytest.raises(MalError, match="level_start_index"):
        msda.check_levels([(6, 20), (3, 10)], [0], 150)
    with pytest.raises(MalError, match="S = 161"):
        msda.check_levels([(6, 20), (3, 10), (2, 5)], [0, 120, 150], 161)
    with pytest.raises(MalError, match="1x1"):
        msda.check_levels([(0, 20)], [0], 0)


def test_module_state_dict_is_upstreams():
    d = R.load_case("m2")
    m = msda.MSDeformAttn(**R.MODULE_CFG)
    sd = m.state_dict()
    assert list(sd) == d["state_keys"] == list(R.STATE_KEYS)
    assert [list(v.shape) for v in sd.values()] == [[int(s) for s in row if s] for row in d["state_shapes"]]
    m.load_state_dict({k: torch.from_numpy(v) for k, v in d["sd"].items()}, strict=True)
    assert m.fused and not msda.MSDeformAttn(**R.MODULE_CFG, fused=False).fused
    # upstream's initial state (ops/modules/ms_deform_attn.py:66-80): zero offset and attention weights, offset biases
    # along direction 2 pi m / M with point i at i + 1 steps
    f = msda.MSDeformAttn(d_model=32, n_levels=2, n_heads=8, n_points=3)
    assert not f.sampling_offsets.weight.any() and not f.attention_weights.weight.any() and not f.attention_weights.bias.any()
    b = f.sampling_offsets.bias.detach().view(8, 2, 3, 2)
    assert torch.allclose(b[0, :, :, 0], torch.tensor([1.0, 2.0, 3.0]).expand(2, 3)) and torch.allclose(b[0, :, :, 1], torch.zeros(2, 3), atol=1e-6)
    assert torch.allclose(b[2, 1, :, 1], torch.tensor([1.0, 2.0, 3.0])) and torch.allclose(b[1, 0, 0], torch.tensor([1.0, 1.0]))


def test_package_exports():
    import mal_amd
    assert mal_amd.MSDeformAttn is msda.MSDeformAttn and mal_amd.ms_deform_attn is msda.ms_deform_attn
    assert {"MSDeformAttn", "ms_deform_attn"} <= set(mal_amd.__all__)
