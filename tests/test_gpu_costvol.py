"""GPU parity of the cost-volume kernels (mal_cost_volume through mal_amd.costvol) against the golden run that used
the reference's layer objects (tests/golden/costvol_*.npz) and, at MAL's size (B=12, 96 bins, 48x160), against
the CPU checker.  fp32; tolerance 1e-4 (north_star) on the volume -- a 1-ulp difference of a sampling position times the feature
gradient is ~1e-5, and the 64-channel mean is summed in a different order -- and
pixels whose sampling position is within 1e-4 of a border-mask threshold or of the image border may fall on
either side (resnet_encoder.py:199-205 compares fp32 positions with 2.0 / w-2)."""
import numpy as np
import pytest
import torch

from tests.costvol_checks import check
from tests.test_costvol_oracle import CASES, load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


@pytest.mark.parametrize("impl", [1, 0], ids=["lane_pixel", "lane_channel"])
@pytest.mark.parametrize("tag", CASES)
def test_golden(tag, impl):
    """both formulations of the match kernel (mal_set_option("costvol_impl"): 1 = planar features, lane = pixel, the
    default; 0 = channel-last, lane = channel) against the golden run"""
    from mal_amd import _lib
    t = torch.from_numpy
    z, cur, look, poses, K, invK, bins = load(tag)
    lib = _lib.load()
    _lib.check(lib.mal_set_option(b"costvol_impl", impl), "costvol_impl")
    try:
        check(cur, look, poses, K, invK, bins, (t(z["out/cost_volume"]), t(z["out/missing"]), t(z["out/masked_cost_volume"]),
                                                t(z["out/lowest_cost"]), t(z["out/confidence"])))
    finally:
        lib.mal_set_option(b"costvol_impl", 1)


def test_mal_size_against_the_cpu_checker():
    from oracle import costvol_oracle as CO
    from oracle.gen_golden_costvol import make_case
    B, F_, C, h, w, D = 12, 1, 64, 48, 160, 96
    cur, look, poses, K, invK = make_case(B, F_, C, h, w, D, seed=5)
    poses = poses.clone()
    poses[:, :, :3, 3] *= 0.25  # gentler motion: most bins land inside
    bins = CO.depth_bins(0.5, 20.0, D, "linear")
    with torch.no_grad():
        cv, miss = CO.match_features(cur, look, poses, K, invK, bins, True)
        masked, low, conf = CO.encoder_outputs(cv, miss, bins)
    assert 0.05 < float(conf.mean()) < 1.0
    check(cur, look, poses, K, invK, bins, (cv, miss, masked, low, conf))
