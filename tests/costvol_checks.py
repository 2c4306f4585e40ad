"""What the cost-volume GPU tests share (tests/test_gpu_costvol.py, tests/test_gpu_costvol_sweep.py): the ambiguity band of
the border mask and the comparison of ``mal_amd.costvol``'s five outputs with a CPU reference.  fp32; tolerance 1e-4
(north_star) on the volume -- a 1-ulp difference of a sampling position times the feature gradient is ~1e-5, and the
64-channel mean is summed in a different order -- and pixels whose sampling position is within 2e-4 px of a border-mask
threshold may fall on either side (resnet_encoder.py:199-205 compares fp32 positions with 2.0 / w-2)."""
import torch

DEV = "cuda:0"


def ambiguous(poses, K, invK, bins, B, h, w, tol=2e-4):
    """(B,D,h,w) bool: the sampling position of (pixel, bin) in ANY frame lies within tol px of 2, w-2, h-2"""
    from oracle import mal_oracle as O
    D = bins.numel()
    amb = torch.zeros(B, D, h, w, dtype=torch.bool)
    depth = bins.view(D, 1, 1, 1).expand(D, 1, h, w).contiguous().double()
    for b in range(B):
        world = O.backproject_depth(depth, invK[b:b + 1].double().expand(D, 4, 4))
        for f in range(poses.shape[1]):
            pix = O.project_3d(world, K[b:b + 1].double().expand(D, 4, 4), poses[b:b + 1, f].double().expand(D, 4, 4), h, w)
            x, y = (pix[..., 0] / 2 + 0.5) * (w - 1), (pix[..., 1] / 2 + 0.5) * (h - 1)
            near = lambda v, t: (v - t).abs() <= tol
            amb[b] |= near(x, 2.0) | near(x, w - 2.0) | near(y, 2.0) | near(y, h - 2.0)
    return amb


def bin_index(lowest_cost, bins):
    """(B,h,w) long: the bin whose depth ``lowest_cost`` = 1 / depth names (the bins are distinct)"""
    return (1 / lowest_cost).unsqueeze(1).sub(bins.view(1, -1, 1, 1)).abs().argmin(1)


def run_gpu(cur, look, poses, K, invK, bins, set_missing_to_max=True):
    """the wrapper's two public functions on the device -> (cv, miss, masked, low, conf) on the CPU"""
    from mal_amd import costvol
    d = lambda t: t.to(DEV)
    cv, miss = costvol.match_features(d(cur), d(look), d(poses), d(K), d(invK), bins, set_missing_to_max)
    masked, low, conf = costvol.cost_volume_outputs(d(cur), d(look), d(poses), d(K), d(invK), bins, set_missing_to_max)
    return cv.cpu(), miss.cpu(), masked.cpu(), low.cpu(), conf.cpu()


def check(cur, look, poses, K, invK, bins, ref, set_missing_to_max=True, amb=None, max_amb_px=None):
    """``ref`` = (cost_volume, missing, masked volume, lowest_cost, confidence) of the CPU reference.  A case may exclude
    at most 2 % of its pixels as ambiguous (``max_amb_px``: that many pixels instead, for shapes where 2 % is about one
    pixel); ``amb``: ``ambiguous(...)`` of the same inputs if the caller already has it.  Returns the device outputs."""
    B, _, h, w = cur.shape
    cv, miss, masked, low, conf = got = run_gpu(cur, look, poses, K, invK, bins, set_missing_to_max)
    if amb is None:
        amb = ambiguous(poses, K, invK, bins, B, h, w)
    amb_px = amb.any(1)                       # a flipped bin changes the pixel's max / confidence / argmin
    ok = ~amb_px.unsqueeze(1).expand_as(amb)
    r_cv, r_miss, r_masked, r_low, r_conf = ref
    if max_amb_px is None:
        assert amb_px.float().mean() <= 0.02
    else:
        assert int(amb_px.sum()) <= max_amb_px
    assert (cv - r_cv)[ok].abs().max() <= 1e-4 * max(1.0, float(r_cv.abs().max()))
    assert torch.equal(miss[ok], r_miss[ok])
    assert (masked - r_masked)[ok].abs().max() <= 1e-4 * max(1.0, float(r_cv.abs().max()))
    assert torch.equal(conf[~amb_px], r_conf[~amb_px])
    # lowest_cost: the argmin may differ where two bins tie to 1e-5; compare the cost AT the chosen bin
    pick = lambda vol, lowc: torch.gather(torch.where(vol == 0, torch.full_like(vol, 100.0), vol), 1,
                                          bin_index(lowc, bins).unsqueeze(1))[:, 0]
    a, bq = pick(r_cv, low), pick(r_cv, r_low)
    assert ((a - bq).abs() <= 2e-4 * bq.abs().clamp(min=1.0))[~amb_px].all()
    return got
