"""DynamicDepth's occlusion-aware cost volume on the device (``mal_cost_volume_dyn``) against the reference's
fixtures and the fp64 restatement (tests/dyn_costvol_restated.py).

Gate (tests/costvol_checks.py): 1e-4 absolute on the UNFILLED volume and the exact missing mask outside an ambiguity set taken
per CELL -- a cell of the (2r+1)^3 window samples the occlusion image within 2e-4 of pool_th, or the cell's own sampling position
lies in the border band; at most 2 % of the cells (tests/test_dyn_costvol_cases.py proves every case decidable within that cap
from the restatements alone).  The filled volume, the confidence and lowest_cost are held EXACTLY to what the fill rule and
``oracle.costvol_oracle.encoder_outputs`` give on the kernel's own unfilled volume."""
import functools

import numpy as np
import pytest
import torch

from tests import dyn_costvol_restated as R
from tests.costvol_checks import DEV

pytestmark = pytest.mark.gpu

AMB_CAP = 0.02
VOL_TOL = 1e-4


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def args_of(c, dev=DEV):
    d = lambda t: t.to(dev)
    return [d(c[k]) for k in ("cur", "look", "poses", "K", "invK", "images", "bins")]


def opts_of(c, dev=DEV):
    return dict(cv_min=c["cv_min"], aug_mask=c["aug"].to(dev), set_1=c["set_1"], pool=c["pool"], pool_r=c["pool_r"], pool_th=c["pool_th"])


def run_gpu(c, set_missing_to_max=False, **over):
    from mal_amd import costvol
    o = opts_of(c)
    o.update(over)
    cv, miss = costvol.match_features_dynamic(*args_of(c), set_missing_to_max=set_missing_to_max, **o)
    return cv.cpu(), miss.cpu()


@functools.lru_cache(maxsize=None)
def reference(name, golden):
    """the case, the fp64 restatement of its unfilled volume and its ambiguous cells -- computed once, shared, never changed"""
    c = R.load_golden(name)[0] if golden else R.sweep_case(name)
    cv64, miss64, mv = R.run_case(c, torch.float64, set_missing_to_max=False, details=True)
    return c, cv64, miss64, R.ambiguous_cells(c, mv)


def gate(name, golden):
    c, cv64, miss64, amb = reference(name, golden)
    cv, miss = run_gpu(c)
    ok = ~amb
    share = float(amb.float().mean())
    err = float((cv.double() - cv64)[ok].abs().max()) if ok.any() else 0.0
    flips = int((miss.double() != miss64)[ok].sum())
    print("%s: ambiguous %.3f %% of the cells, volume error %.2e, %d missing cells differ" % (name, 100 * share, err, flips))
    assert share <= AMB_CAP
    assert err <= VOL_TOL * max(1.0, float(cv64.abs().max()))
    assert flips == 0
    return c, cv, miss


def filled_outputs_follow_the_unfilled_volume(c, cv_u, miss_u):
    """set_missing_to_max=True: volume, missing mask, volume x confidence, lowest_cost and confidence, bit for bit from the
    kernel's own unfilled volume"""
    from mal_amd import costvol
    from oracle import costvol_oracle as CO
    cv_f, miss_f = run_gpu(c, set_missing_to_max=True)
    masked, low, conf = [t.cpu() for t in costvol.cost_volume_outputs_dynamic(*args_of(c), set_missing_to_max=True, **opts_of(c))]
    assert torch.equal(miss_u, (cv_u == 0).float()) and torch.equal(miss_f, miss_u)
    want = cv_u * (1 - miss_u) + cv_u.max(1)[0].unsqueeze(1) * miss_u
    assert np.array_equal(bits(cv_f), bits(want))
    w_masked, w_low, w_conf = CO.encoder_outputs(want, miss_u, c["bins"])
    assert np.array_equal(bits(masked), bits(w_masked)) and np.array_equal(bits(conf), bits(w_conf))
    assert np.array_equal(bits(low), bits(w_low))


@pytest.mark.parametrize("name", R.GOLDEN_CASES)
def test_reference_fixtures(name):
    """the ten reference files: the fp64 gate, and the reference's own fp32 volume to the same tolerance"""
    c, cv, miss = gate(name, True)
    _, r_cv, r_miss = R.load_golden(name)          # filled, fp32
    _, _, _, amb = reference(name, True)
    cv_f, miss_f = run_gpu(c, set_missing_to_max=True)
    ok = ~amb.any(1, keepdim=True).expand_as(amb)  # a flipped cell moves the pixel's maximum, which fills its missing bins
    assert (cv_f - r_cv)[ok].abs().max() <= VOL_TOL * max(1.0, float(r_cv.abs().max()))
    assert torch.equal(miss_f[ok], r_miss[ok])
    if name.endswith(("default", "set_1")):
        filled_outputs_follow_the_unfilled_volume(c, cv, miss)


@pytest.mark.parametrize("name", list(R.SWEEP))
def test_sweep_against_the_restatement(name):
    c, cv, miss = gate(name, False)
    filled_outputs_follow_the_unfilled_volume(c, cv, miss)
    if name == "set_1_zero_feats":
        assert bool((miss[0, :, 3, 3] == 1).all())  # a cost of exactly 1 reads as missing
    if name == "th_below_0":  # every cell masked, every neighbour too: the pooled value is 0 on every channel
        want = c["cur"].abs().mean(1)[:, None].expand_as(cv)
        hit = cv != 0
        assert hit.any() and float((cv - want)[hit].abs().max()) <= 1e-5  # 64 terms of ~0.4 summed in another order


def test_pool_moves_the_volume():
    """the case of tests/test_dyn_costvol_cases.py in which the pool changes > 5 % of the cells: so it does on the device"""
    c = reference("D96_16x28", False)[0]
    a, b = run_gpu(c)[0], run_gpu(c, pool=False)[0]
    assert float((a != b).float().mean()) > 0.05


# ---- properties, bitwise
def test_averaging_without_dark_pixels_is_mal_cost_volume():
    from mal_amd import costvol
    for name in ("no_black", "D96_16x28", "D7_16x28"):
        c = dict(reference(name, False)[0])
        if name != "no_black":
            c["images"] = c["images"].clamp(min=0.1)
        for fill in (False, True):
            a = args_of(c)
            want = costvol.match_features(*a[:5], a[6], set_missing_to_max=fill)
            for o in (dict(pool=True, set_1=False), dict(pool=False, set_1=True), dict(pool=False, set_1=False)):
                got = costvol.match_features_dynamic(*a, set_missing_to_max=fill, **dict(opts_of(c), cv_min=False, **o))
                assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))


def test_augmented_samples_get_the_options_off_result():
    for name in ("D7_16x28", "mean_r2", "set_1_zero_feats"):
        c = reference(name, False)[0]
        ones = torch.ones_like(c["aug"]).to(DEV)
        a, b = run_gpu(c, aug_mask=ones), run_gpu(c, pool=False, set_1=False)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
        mixed = run_gpu(c, aug_mask=None)  # None = all zero: no sample is augmented
        full = run_gpu(c, aug_mask=torch.zeros_like(ones))
        assert np.array_equal(bits(mixed[0]), bits(full[0]))


def test_the_threshold_is_strict():
    """without a dark pixel every sampled occlusion value is exactly 0 in any precision: at pool_th = 0 a strict test masks
    nothing (the options-off result, bit for bit), a >= would mask every cell"""
    c = reference("no_black", False)[0]
    off = run_gpu(c, pool=False, set_1=False)
    for o in (dict(pool=True, set_1=False, pool_r=1), dict(pool=False, set_1=True)):
        got = run_gpu(c, pool_th=0.0, **o)
        assert np.array_equal(bits(got[0]), bits(off[0])) and np.array_equal(bits(got[1]), bits(off[1]))
    assert not np.array_equal(bits(run_gpu(c, pool_th=-0.5)[0]), bits(off[0]))  # the case can tell: below 0 everything is masked


def test_two_runs_are_equal():
    for name in ("D96_16x28", "F3_occ_b"):
        c = reference(name, False)[0]
        a, b = run_gpu(c), run_gpu(c)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


def test_graph_replay_equals_the_eager_call():
    """one stream, one branch: the call reads aug_mask and the zero pose on the device, so the captured call follows inputs
    rewritten between replays"""
    from mal_amd import costvol
    c = reference("D7_16x28", False)[0]
    a, o = args_of(c), opts_of(c)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        costvol.match_features_dynamic(*a, **o)  # warm
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            cv, miss = costvol.match_features_dynamic(*a, **o)
            masked, low, conf = costvol.cost_volume_outputs_dynamic(*a, **o)
    torch.cuda.current_stream().wait_stream(s)
    aug0, pose0 = o["aug_mask"].clone(), a[2].clone()
    for aug, zero in ((aug0, None), (1 - aug0, None), (aug0, (1, 0)), (torch.zeros_like(aug0), (0, 2))):
        o["aug_mask"].copy_(aug)
        a[2].copy_(pose0)
        if zero:
            a[2][zero[0], zero[1]] = 0.0
        graph.replay()
        torch.cuda.synchronize()
        e_cv, e_miss = costvol.match_features_dynamic(*a, **o)
        e_masked, e_low, e_conf = costvol.cost_volume_outputs_dynamic(*a, **o)
        for x, y in ((cv, e_cv), (miss, e_miss), (masked, e_masked), (low, e_low), (conf, e_conf)):
            assert np.array_equal(bits(x), bits(y))


# ---- refusals
def test_refusals():
    from mal_amd import costvol
    from mal_amd._lib import MalError
    c = reference("D3_8x8", False)[0]
    with pytest.raises(MalError, match="--cv_pool_radius"):
        costvol.match_features_dynamic(*args_of(c), **dict(opts_of(c), pool_r=3))
    a = args_of(c)
    a[0], a[1] = a[0][:, :32].contiguous(), a[1][:, :, :32].contiguous()
    with pytest.raises(MalError):
        costvol.match_features_dynamic(*a, **opts_of(c))
    with pytest.raises(MalError, match="no CPU fallback"):
        costvol.match_features_dynamic(*args_of(c, "cpu"), **opts_of(c, "cpu"))
    with pytest.raises(MalError):  # the occlusions are read from the lookup images
        a = args_of(c)
        a[5] = None
        costvol.match_features_dynamic(*a, **opts_of(c))


def test_c_abi_refuses_before_any_launch():
    from mal_amd import _lib as L
    lib = L.load()
    EINVAL, ESHAPE = -1, -2  # include/mal_hip.h
    assert lib.mal_cost_volume_dyn_workspace_bytes(2, 2, 96, 12, 20) >= 2 * 2 * 48 * 128 + 2 * 2 * 96 * 12 * 20
    assert lib.mal_cost_volume_dyn_workspace_bytes(2, 2, 257, 12, 20) == 0 and lib.mal_cost_volume_dyn_workspace_bytes(2, 2, 96, 4, 20) == 0
    x = torch.zeros(1 << 16, device=DEV)
    p = x.data_ptr()
    call = lambda C, D, h, r, ws, wsb: lib.mal_cost_volume_dyn(p, p, p, p, p, p, 1, 1, C, D, h, 8, 1e-7, 1, p, 32, 32, None, 1, 0, 1, r, 0.4, p,
                                                                None, None, None, None, ws, wsb, None)
    assert call(32, 4, 8, 1, p, 1 << 18) == ESHAPE and call(64, 257, 8, 1, p, 1 << 18) == ESHAPE
    assert call(64, 4, 4, 1, p, 1 << 18) == ESHAPE
    assert call(64, 4, 8, 3, p, 1 << 18) == EINVAL and call(64, 4, 8, -1, p, 1 << 18) == EINVAL
    assert call(64, 4, 8, 1, None, 0) == EINVAL and call(64, 4, 8, 1, p, 16) == EINVAL
    torch.cuda.synchronize()


def test_encoder_forward_runs_and_follows_its_options():
    from mal_amd import networks as N
    torch.manual_seed(0)
    enc = N.DynamicDepthEncoderMatching(18, False, 64, 96, min_depth_bin=0.4, max_depth_bin=9.0, num_depth_bins=8).to(DEV).eval()
    c = R.make_case(2, 2, 16, 24, 8, seed=40, aug=[0, 0])
    g = torch.Generator().manual_seed(3)
    cur_img = torch.rand(2, 3, 64, 96, generator=g).to(DEV)
    look_img = c["images"].reshape(2, 2, 3, 64, 96).to(DEV)
    d = lambda k: c[k].to(DEV)
    with torch.no_grad():
        f_pool, low, conf = enc(cur_img, look_img, d("poses"), d("K"), d("invK"), cv_min=True, aug_mask=d("aug"), pool=True, pool_r=1, pool_th=0.7)
        f_pool = [t.clone() for t in f_pool]
        f_off, _, _ = enc(cur_img, look_img, d("poses"), d("K"), d("invK"), cv_min=True, aug_mask=1 - d("aug"), pool=True, pool_r=1, pool_th=0.7)
    assert len(f_pool) == 5 and low.shape == (2, 16, 24) and conf.shape == (2, 16, 24)
    assert all(bool(torch.isfinite(t).all()) for t in f_pool)
    assert torch.equal(f_pool[0], f_off[0]) and torch.equal(f_pool[1], f_off[1])  # before the cost volume
