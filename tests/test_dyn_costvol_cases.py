"""CPU side of DynamicDepth's occlusion-aware cost volume: the torch restatement against the reference's
fixtures, the nearest-resize rule the occlusion-image kernel uses, and the proof -- from the fp32 and fp64 restatements alone
-- that every case of the GPU sweep (tests/test_gpu_dyn_costvol.py) can be held to its gate within its caps."""
import functools
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dyn_costvol_restated as R

AMB_CAP = 0.02   # share of CELLS a case may exclude as ambiguous
VOL_TOL = 1e-4   # tests/costvol_checks.py


@pytest.mark.parametrize("name", R.GOLDEN_CASES)
def test_restatement_equals_the_reference_bit_for_bit(name):
    c, cv, miss = R.load_golden(name)
    assert c["bins"].numel() == 96 and c["cur"].shape[1] == 64
    got_cv, got_miss = R.run_case(c, torch.float32)
    assert np.array_equal(got_cv.numpy().view(np.int32), cv.numpy().view(np.int32))
    assert torch.equal(got_miss, miss)


def test_fixtures_cover_the_option_rows_a_zero_pose_and_an_augmented_sample():
    c, _, _ = R.load_golden("b2_f2_12x20_default")
    assert float(c["poses"][0, 1].abs().sum()) == 0 and float(c["poses"][0, 0].abs().sum()) > 0
    assert c["aug"].reshape(-1).tolist() == [0.0, 1.0]
    rows = {tuple(R.load_golden("b1_f1_9x70_" + o)[0][k] for k in ("cv_min", "set_1", "pool", "pool_r", "pool_th")) for o in R.OPTION_ROWS}
    assert rows == {(True, False, True, 1, 0.7), (True, False, True, 2, 0.4), (True, True, False, 2, 0.4),
                    (False, False, True, 1, 0.7), (True, False, False, 2, 0.4)}


@pytest.mark.parametrize("H,W", [(37, 50), (200, 130), (20, 28), (192, 512), (48, 128), (96, 256), (24, 64), (1, 1), (47, 129),
                                 (49, 127), (333, 1000)])
def test_nearest_resize_rule_is_atens(H, W):
    """the source index of every cell of the 48x128 occlusion image, as the kernel computes it, against F.interpolate"""
    src = torch.arange(H * W, dtype=torch.float32).reshape(1, 1, H, W)  # every source pixel is its own index (exact below 2^24)
    ref = F.interpolate(src, [R.OCC_H, R.OCC_W])[0, 0].long()
    iy, ix = R.nearest_source_index(R.OCC_H, H), R.nearest_source_index(R.OCC_W, W)
    assert np.array_equal(ref.numpy(), iy[:, None] * W + ix[None, :])
    g = torch.Generator().manual_seed(H * 1000 + W)
    img = R.make_images(2, H, W, g, holes=0.05)
    assert torch.equal(R.occlusion_images(img), F.interpolate((img.sum(1).unsqueeze(1) < 0.15).float(), [R.OCC_H, R.OCC_W])[:, 0])


def test_case_images_have_no_near_tie_at_the_darkness_test():
    for name in R.SWEEP:
        img = R.sweep_case(name)["images"]
        dark = img.sum(1) < 0.15
        assert (img.amax(1)[dark] <= 0.04).all() and (img.amin(1)[~dark] >= 0.1).all()


@functools.lru_cache(maxsize=None)
def _both(name):
    c = R.sweep_case(name)
    cv32, miss32 = R.run_case(c, torch.float32, set_missing_to_max=False)
    cv64, miss64, mv = R.run_case(c, torch.float64, set_missing_to_max=False, details=True)
    return c, cv32, miss32, cv64, miss64, R.ambiguous_cells(c, mv)


@pytest.mark.parametrize("name", list(R.SWEEP))
def test_sweep_case_is_decidable_within_its_caps(name):
    """the reference's own fp32 against fp64 passes the GPU gate: at most 2 % of the cells are ambiguous and, outside them,
    the missing cells are the same and the volume agrees to 1e-4"""
    c, cv32, miss32, cv64, miss64, amb = _both(name)
    share = float(amb.float().mean())
    ok = ~amb
    diff = float((cv32.double() - cv64)[ok].abs().max()) if ok.any() else 0.0
    print("%s: ambiguous %.3f %%, volume fp32 vs fp64 %.2e, missing %.1f %%" % (name, 100 * share, diff, 100 * float(miss64.mean())))
    assert share <= AMB_CAP
    assert torch.equal(miss32[ok].double(), miss64[ok])
    assert diff <= VOL_TOL * max(1.0, float(cv64.abs().max()))


def test_sweep_covers_what_it_claims():
    a = {n: R.SWEEP[n][0] for n in R.SWEEP}
    assert {v["D"] for v in a.values()} >= {1, 2, 3, 5, 7, 13, 96, 100}
    assert {(v["h"], v["w"]) for v in a.values()} >= {(5, 13), (7, 9), (8, 8), (5, 70), (16, 28)}
    assert {v["F_"] for v in a.values()} == {1, 2, 3}
    assert {R.SWEEP[n][1]["pool_r"] for n in R.SWEEP if R.SWEEP[n][1]["pool"]} == {0, 1, 2}
    assert any(R.SWEEP[n][1]["pool_th"] < 0 for n in R.SWEEP) and any(R.SWEEP[n][1]["pool_th"] >= 1 for n in R.SWEEP)
    assert any("HW" in v for v in a.values())
    assert bool((R.sweep_case("all_black")["images"].sum(1) < 0.15).all())
    assert not bool((R.sweep_case("no_black")["images"].sum(1) < 0.15).any())


def test_all_masked_and_none_masked_thresholds_do_what_they_say():
    _, _, _, _, _, _ = _both("th_below_0")
    c = R.sweep_case("th_below_0")
    mv = R.run_case(c, torch.float64, details=True)[2]
    assert bool((mv[~mv.isnan()] > c["pool_th"]).all())
    c = R.sweep_case("th_above_1")
    mv = R.run_case(c, torch.float64, details=True)[2]
    assert not bool((mv[~mv.isnan()] > c["pool_th"]).any())
    assert torch.allclose(R.run_case(c)[0], R.run_case(c, pool=False)[0], rtol=0, atol=1e-6)  # torch's own mean order differs by an ulp


def test_the_threshold_is_strict():
    """the tie the GPU file uses: no dark pixel, pool_th = 0 -- every sampled value is exactly 0 and nothing is masked"""
    c = R.sweep_case("no_black")
    mv = R.run_case(c, torch.float32, details=True, pool_th=0.0)[2]
    assert bool((mv[~mv.isnan()] == 0).all())
    off = R.run_case(c, pool=False)[0]
    assert torch.allclose(R.run_case(c, pool_th=0.0)[0], off, rtol=0, atol=1e-6)
    assert float((R.run_case(c, pool_th=-0.5)[0] - off).abs().max()) > 1e-3


def test_set_1_on_zero_features_reads_as_missing():
    c, _, _, cv64, miss64, _ = _both("set_1_zero_feats")
    assert bool((miss64[0, :, 3, 3] == 1).all()) and bool((cv64[0, :, 3, 3] == 0).all())
    assert float(miss64[0, :, 4, 4].min()) == 0  # its neighbour has features: a cost below 1


def test_the_occ_b_rule_matters_in_a_listed_case():
    c = R.sweep_case("F3_occ_b")
    a = R.run_case(c, set_missing_to_max=False)[0]
    args = [c[k] for k in ("cur", "look", "poses", "K", "invK", "images", "bins", "cv_min", "aug", "set_1", "pool", "pool_r", "pool_th")]
    F_ = c["look"].shape[1]
    b = R.match_features(*args, set_missing_to_max=False, occ_index=lambda b, f: b * F_ + f)[0]
    assert float((a != b).float().mean()) > 0.01


def test_pool_changes_more_than_five_percent_of_a_listed_case():
    """a kernel that ignores the pool cannot pass: against cv_min alone the pooled fill moves > 5 % of the cells"""
    c, cv, _ = R.load_golden("b2_f2_12x20_default")
    plain = R.load_golden("b2_f2_12x20_cv_min")[1]
    share = float((cv != plain).float().mean())
    print("pool changes %.1f %% of the cells of b2_f2_12x20" % (100 * share))
    assert share > 0.05
    c = R.sweep_case("D96_16x28")
    share = float((R.run_case(c, set_missing_to_max=False)[0] != R.run_case(c, set_missing_to_max=False, pool=False)[0]).float().mean())
    print("pool changes %.1f %% of the cells of D96_16x28" % (100 * share))
    assert share > 0.05


def test_python_refuses_a_wide_pool_by_option_name():
    from mal_amd import costvol
    from mal_amd._lib import MalError
    z = torch.zeros(1, 64, 8, 8)
    for fn in (costvol.match_features_dynamic, costvol.cost_volume_outputs_dynamic):
        with pytest.raises(MalError, match="--cv_pool_radius"):
            fn(z, z.unsqueeze(1), torch.eye(4).view(1, 1, 4, 4), torch.eye(4)[None], torch.eye(4)[None], torch.zeros(1, 3, 32, 32),
               torch.linspace(1, 2, 4), pool=True, pool_r=3)
        sig = inspect.signature(fn)
        assert list(sig.parameters)[:7] == ["current_feats", "lookup_feats", "relative_poses", "K", "invK", "lookup_images", "depth_bins"]
        assert {k: sig.parameters[k].default for k in ("cv_min", "aug_mask", "set_1", "pool", "pool_r", "pool_th")} == \
            dict(cv_min=True, aug_mask=None, set_1=False, pool=False, pool_r=2, pool_th=0.4)


def test_encoder_class_has_upstreams_signature_and_its_parents_parameters():
    from mal_amd import networks as N
    sig = inspect.signature(N.DynamicDepthEncoderMatching.forward)
    assert list(sig.parameters) == ["self", "current_image", "lookup_images", "poses", "K", "invK", "min_depth_bin", "max_depth_bin",
                                    "teacher_depth", "mask_noise", "doj_mask", "cv_min", "aug_mask", "set_1", "pool", "pool_r", "pool_th"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(min_depth_bin=None, max_depth_bin=None, teacher_depth=None, mask_noise=False, doj_mask=None, cv_min=True,
                     aug_mask=None, set_1=False, pool=False, pool_r=2, pool_th=0.4)
    kw = dict(num_layers=18, pretrained=False, input_height=64, input_width=96, num_depth_bins=8)
    torch.manual_seed(0)
    a = N.ResnetEncoderMatching(**kw)
    torch.manual_seed(0)
    b = N.DynamicDepthEncoderMatching(**kw)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert list(inspect.signature(N.ResnetEncoderMatching.forward).parameters) == ["self", "current_image", "lookup_images", "poses", "K",
                                                                                   "invK", "min_depth_bin", "max_depth_bin"]
