"""The cost-volume kernels (mal_cost_volume, mal_amd/csrc/mal_costvol.hip, through mal_amd.costvol) swept over what they
branch on: the bin count against the three ways the kernels partition it (groups of 6, rounds of 64, four LDS parts), image
sizes at the edges of the launch geometry (64 pixels per wave, 256 per workgroup, 64 per finish workgroup), the number of
lookup frames, missing frames and samples, the bin schedules, ``set_missing_to_max``, exact ties of the first-minimum rule,
and the sixteen combinations of nullable outputs -- both formulations (``costvol_impl`` 1 and 0) each time.

Inputs: ``oracle.gen_golden_costvol.make_case(seed=5)`` with translations x 0.25 (as the MAL-size test of
tests/test_gpu_costvol.py); expected values: ``oracle.costvol_oracle`` on the CPU, computed once per case and shared by the
two formulations.  Tolerances are those of ``tests.costvol_checks.check``: 1e-4 x max(1, max|cv|) on the volumes, exact
``missing`` / ``confidence`` outside the 2e-4 px ambiguity band, at most 2 % of a case's pixels excluded as ambiguous."""
import contextlib
import functools
import itertools
import types

import pytest
import torch

from oracle import costvol_oracle as CO
from tests.costvol_checks import DEV, ambiguous, bin_index, check, run_gpu

pytestmark = pytest.mark.gpu
both_formulations = pytest.mark.parametrize("impl", [1, 0], ids=["lane_pixel", "lane_channel"])
C = 64


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


@contextlib.contextmanager
def formulation(impl):
    """mal_set_option("costvol_impl"): 1 = planar features, lane = pixel (default); 0 = channel-last, lane = channel"""
    from mal_amd import _lib
    lib = _lib.load()
    _lib.check(lib.mal_set_option(b"costvol_impl", impl), "costvol_impl")
    try:
        yield lib
    finally:
        lib.mal_set_option(b"costvol_impl", 1)


@functools.lru_cache(maxsize=None)
def inputs(B, F_, h, w):
    """(cur, look, poses, K, invK); callers clone what they change"""
    from oracle.gen_golden_costvol import make_case
    cur, look, poses, K, invK = make_case(B, F_, C, h, w, 0, seed=5)  # (make_case does not read its bin count)
    poses = poses.clone()
    poses[:, :, :3, 3] *= 0.25  # gentler motion: most bins land inside
    return cur, look, poses, K, invK


def linear(D):
    return CO.depth_bins(0.5, 20.0, D, "linear")


def reference(ins, bins, set_missing_to_max=True):
    with torch.no_grad():
        cv, miss = CO.match_features(*ins, bins, set_missing_to_max)
        masked, low, conf = CO.encoder_outputs(cv, miss, bins)
    return cv, miss, masked, low, conf


@functools.lru_cache(maxsize=None)
def case(B, F_, h, w, D, binning="linear", set_missing_to_max=True):
    """a make_case input with its bins, CPU reference and ambiguity band: computed once, shared by the two formulations"""
    ins = inputs(B, F_, h, w)
    bins = CO.depth_bins(0.5, 20.0, D, binning)
    return ins, bins, reference(ins, bins, set_missing_to_max), ambiguous(ins[2], ins[3], ins[4], bins, B, h, w)


def inner_missing_share(ref):
    return float(ref[1][:, :, 2:-2, 2:-2].mean())


# ------------------------------------------------------------------ 1. bin counts
# next to the multiples of kCvG = 6 and of 64, below 4 (empty finish parts), not multiples of 4, rounds 3 and 4, the maximum
BIN_COUNTS = [1, 2, 3, 4, 5, 6, 7, 12, 13, 63, 64, 65, 127, 128, 129, 192, 255, 256]


@both_formulations
@pytest.mark.parametrize("D", BIN_COUNTS)
def test_bin_counts(D, impl):
    """23x41 = 943 pixels = 3 x 256 + 175 = 14 x 64 + 47: every kernel has a partial last wave.  B=2, F=2, sample 1 with its
    second frame missing.  The case is not degenerate (from the reference alone): some but not all inner bins are missing
    and, with five bins or more, ``lowest_cost`` takes at least five values."""
    ins, bins, ref, amb = case(2, 2, 23, 41, D)
    assert 0.0 < inner_missing_share(ref) < 1.0
    if D >= 5:
        assert ref[3].unique().numel() >= 5
    with formulation(impl):
        check(*ins, bins, ref, amb=amb)


# ------------------------------------------------------------------ 2. image sizes
SHAPES = [(5, 5), (5, 64), (64, 5), (6, 7), (8, 8), (16, 16), (16, 17), (7, 37), (23, 67)]
TINY = {(5, 5), (6, 7)}


@both_formulations
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes(hw, impl):
    """D=11, B=2, F=2 at the minimum legal size (one inner pixel), one inner row / column, h*w = 64 and 256 exactly and one
    column more, and partial waves.

    Tiny-shape rule: at 5x5 (50 pixels) and 6x7 (84) 2 % of the case is about one pixel, so there the condition is AT MOST
    3 AMBIGUOUS PIXELS IN THE CASE instead of 2 % -- what the reference produces at 5x5 (3 of 50).

    The reference reports every bin missing at 5x5; the case stays for the launch geometry and the all-missing result at
    the smallest size, and it alone is exempt from the non-degeneracy assertion.  That assertion asks here for a missing
    share strictly inside (0, 1) and a ``lowest_cost`` that is not constant: an inner region of 1 x 60 or 2 x 3 pixels
    cannot be asked for the five values of the 943-pixel cases (the reference gives 3 at 16x16, 5 at 6x7)."""
    h, w = hw
    ins, bins, ref, amb = case(2, 2, h, w, 11)
    if hw == (5, 5):
        assert bool((ref[1] == 1).all())
    else:
        assert 0.0 < inner_missing_share(ref) < 1.0
        assert ref[3].unique().numel() >= 2
    with formulation(impl):
        check(*ins, bins, ref, amb=amb, max_amb_px=3 if hw in TINY else None)


# ------------------------------------------------------------------ 3. frames, schedules, the flag
@both_formulations
@pytest.mark.parametrize("F_", [1, 3, 4])
def test_frame_counts(F_, impl):
    ins, bins, ref, amb = case(2, F_, 23, 41, 13)
    assert 0.0 < inner_missing_share(ref) < 1.0 and ref[3].unique().numel() >= 5
    with formulation(impl):
        check(*ins, bins, ref, amb=amb)


@functools.lru_cache(maxsize=None)
def dropped_sample_case():
    cur, look, poses, K, invK = inputs(3, 3, 23, 41)
    poses = poses.clone()
    poses[1] = 0.0
    ins, bins = (cur, look, poses, K, invK), linear(13)
    return ins, bins, reference(ins, bins), ambiguous(poses, K, invK, bins, 3, 23, 41)


@both_formulations
def test_sample_with_every_frame_missing(impl):
    """RepDepth's matching augmentation zeroes all poses of a sample with probability 0.25 per sample and step
    (mal_amd/networks.py, ``dropped``): that sample's volume is 0, every bin missing, confidence 0 and ``lowest_cost`` names
    bin 0 -- exactly; the other two samples go through the full check"""
    ins, bins, ref, amb = dropped_sample_case()
    with formulation(impl):
        cv, miss, masked, low, conf = check(*ins, bins, ref, amb=amb)
    assert not cv[1].any() and not masked[1].any() and not conf[1].any()
    assert bool((miss[1] == 1).all())
    assert not bin_index(low, bins)[1].any()
    assert torch.equal(low[1], ref[3][1])
    assert 0.0 < float(ref[1][[0, 2]][:, :, 2:-2, 2:-2].mean()) < 1.0


@functools.lru_cache(maxsize=None)
def zero_sum_pose_case():
    """identity rotation, translation (-1.5, -1.5, -1.0): 16 entries that are not all zero and sum to exactly 0 in any order.
    Upstream's test for a missing frame is ``pose.sum() == 0`` (resnet_encoder.py:176-178), so the frame is skipped"""
    cur, look, poses, K, invK = inputs(2, 2, 23, 41)
    quirk = torch.eye(4)
    quirk[:3, 3] = torch.tensor([-1.5, -1.5, -1.0])
    assert float(quirk.sum()) == 0.0
    with_quirk, zeroed, live = poses.clone(), poses.clone(), poses.clone()
    with_quirk[0, 0], zeroed[0, 0], live[0, 0] = quirk, 0.0, quirk
    live[0, 0, 0, 3] += 1e-6  # the same frame, not skipped
    bins = linear(13)
    ref = reference((cur, look, with_quirk, K, invK), bins)
    ref_zeroed = reference((cur, look, zeroed, K, invK), bins)
    ref_live = reference((cur, look, live, K, invK), bins)
    return (cur, look, with_quirk, K, invK), zeroed, bins, ref, ref_zeroed, ref_live, ambiguous(zeroed, K, invK, bins, 2, 23, 41)


@both_formulations
def test_pose_whose_entries_sum_to_zero_is_a_missing_frame(impl):
    """a true zero pose projects everything to (0, 0), which the border mask removes anyway: only a non-zero pose whose
    entries sum to zero shows whether the kernels have upstream's ``pose.sum() == 0`` rule.  Bit for bit the run with that
    frame's pose zeroed, and the reference's result"""
    ins, zeroed, bins, ref, ref_zeroed, ref_live, amb = zero_sum_pose_case()
    # the construction, from the reference alone: it skips the frame, and the frame would matter if it were not skipped
    assert all(torch.equal(a, b) for a, b in zip(ref, ref_zeroed))
    assert float((ref_live[0] - ref[0]).abs().max()) > 0.01
    cur, look, poses, K, invK = ins
    with formulation(impl):
        got = check(*ins, bins, ref, amb=amb)
        got_zeroed = run_gpu(cur, look, zeroed, K, invK, bins)
    for a, b in zip(got, got_zeroed):
        assert torch.equal(a, b)


@both_formulations
@pytest.mark.parametrize("binning", ["inverse", "log"])
def test_bin_schedules(binning, impl):
    """24x40, D=96 with the bins ``ResnetEncoderMatching.compute_depth_bins`` makes, which must be the checker's"""
    from mal_amd.networks import ResnetEncoderMatching
    ins, bins, ref, amb = case(2, 2, 24, 40, 96, binning)
    enc = types.SimpleNamespace(depth_binning=binning, num_depth_bins=96, depth_bins=None)
    ResnetEncoderMatching.compute_depth_bins(enc, 0.5, 20.0)
    assert torch.equal(enc.depth_bins, bins)
    assert 0.0 < inner_missing_share(ref) < 1.0 and ref[3].unique().numel() >= 5
    with formulation(impl):
        check(*ins, enc.depth_bins, ref, amb=amb)


@both_formulations
@pytest.mark.parametrize("h,w,D", [(24, 40, 96), (23, 41, 7)])
def test_missing_bins_left_at_zero(h, w, D, impl):
    """``set_missing_to_max=False``: the volume keeps its zeros, which ``lowest_cost`` reads as 100"""
    ins, bins, ref, amb = case(2, 2, h, w, D, "linear", False)
    assert 0.0 < inner_missing_share(ref) < 1.0 and ref[3].unique().numel() >= 5
    assert bool((ref[0][ref[1] == 1] == 0).all())
    with formulation(impl):
        check(*ins, bins, ref, set_missing_to_max=False, amb=amb)


# ------------------------------------------------------------------ 4. exact ties
@functools.lru_cache(maxsize=None)
def tie_case(D):
    """F=1 and ``lookup_feats`` all zeros: every sampled value is +-0, so each hit bin of a pixel costs mean_c |current|,
    summed in the same order for every bin -- all hit bins of a pixel hold bit-identical costs, on the device as in the
    reference.  -> inputs, bins, the first hit bin per pixel (0 where there is none), which pixels have a hit, ambiguity"""
    cur, look, poses, K, invK = inputs(2, 1, 23, 41)
    ins, bins = (cur, torch.zeros_like(look), poses, K, invK), linear(D)
    raw = reference(ins, bins, False)[0]
    hit = raw > 0
    any_hit = hit.any(1)
    inf = torch.full_like(raw, float("inf"))
    assert torch.equal(torch.where(hit, raw, -inf).amax(1)[any_hit], torch.where(hit, raw, inf).amin(1)[any_hit])
    first = torch.where(any_hit, hit.float().argmax(1), torch.zeros(any_hit.shape, dtype=torch.long))
    per = (D + 3) // 4  # the finish kernel's LDS parts
    assert set((first[any_hit] // per).tolist()) == {0, 1, 2, 3}
    assert int((first > 0).sum()) >= 100
    return ins, bins, first, ambiguous(poses, K, invK, bins, 2, 23, 41)


@both_formulations
@pytest.mark.parametrize("set_missing_to_max", [True, False], ids=["filled", "zeros"])
@pytest.mark.parametrize("D", [4, 37, 256])
def test_first_minimum_wins_exact_ties(D, set_missing_to_max, impl):
    """the earlier bin wins a tie, within an LDS part of the finish kernel and across the four (D=4: one bin per part).
    Filled: the missing bins take the same maximum, every bin ties and bin 0 wins at every pixel.  Zeros: they read as 100
    and the first hit bin wins, bin 0 where there is no hit.  The recovered bin index is compared, not the float, at every
    pixel outside the ambiguity band"""
    ins, bins, first, amb = tie_case(D)
    ref = reference(ins, bins, set_missing_to_max)
    viz = torch.where(ref[0] == 0, torch.full_like(ref[0], 100.0), ref[0])
    r_arg = viz.min(1)[1]
    assert torch.equal(r_arg, torch.zeros_like(first) if set_missing_to_max else first)  # the construction worked
    with formulation(impl):
        low = check(*ins, bins, ref, set_missing_to_max=set_missing_to_max, amb=amb)[3]
    keep = ~amb.any(1)
    assert torch.equal(bin_index(low, bins)[keep], r_arg[keep])


# ------------------------------------------------------------------ 5. every output written, nothing else written
PAD = 4096  # sentinel floats before and after each output
OUTPUTS = ("missing", "masked", "lowest", "confidence")


def abi_call(lib, dev_ins, B, F_, D, h, w, want):
    """mal_cost_volume itself, each output inside a larger allocation pre-filled with NaN -> {name: (B,...) output}.
    Asserts that every element of every output was written (finite) and that no sentinel was"""
    from mal_amd import _lib, ops
    n = {"cost": B * D * h * w, "missing": B * D * h * w, "masked": B * D * h * w, "lowest": B * h * w, "confidence": B * h * w}
    big = {k: torch.full((PAD + n[k] + PAD,), float("nan"), device=DEV) for k in n if k == "cost" or want[k]}
    ptr = lambda k: big[k].data_ptr() + 4 * PAD if k in big else None
    args = [t.data_ptr() for t in dev_ins]
    _lib.check(lib.mal_cost_volume(*args, B, F_, C, D, h, w, 1e-7, 1, ptr("cost"), ptr("missing"), ptr("masked"), ptr("lowest"),
                                   ptr("confidence"), ops._stream()), "mal_cost_volume")
    torch.cuda.synchronize()
    out = {}
    for k, t in big.items():
        assert bool(torch.isnan(t[:PAD]).all()) and bool(torch.isnan(t[PAD + n[k]:]).all()), k
        out[k] = t[PAD:PAD + n[k]].clone()
        assert bool(torch.isfinite(out[k]).all()), k
    return out


@both_formulations
@pytest.mark.parametrize("D", [7, 65])
def test_every_output_written_and_nothing_else(D, impl):
    """the wrapper allocates with torch.empty, so an element a call skips is silent garbage.  All sixteen null / non-null
    combinations of the four optional outputs: every requested output is written completely, bit-identical to the
    all-outputs run (no atomics: run-to-run equality is exact), ``cost_volume`` is the same in all sixteen, the sentinels
    around every buffer survive; the all-outputs run is the wrapper's result, and on the border rows and columns exactly
    the reference's (zeros, every bin missing, bin 0)"""
    B, F_, h, w = 2, 2, 23, 41
    (cur, look, poses, K, invK), bins, ref, _ = case(B, F_, h, w, D)
    with formulation(impl) as lib:
        wrapper = run_gpu(cur, look, poses, K, invK, bins)
        if lib.mal_costvol_channel_last():
            cur_d, look_d = cur.permute(0, 2, 3, 1).contiguous().to(DEV), look.permute(0, 1, 3, 4, 2).contiguous().to(DEV)
        else:
            cur_d, look_d = cur.to(DEV), look.to(DEV)
        dev_ins = [cur_d, look_d, poses.reshape(B, F_, 16).to(DEV), K.reshape(B, 16).to(DEV), invK.reshape(B, 16).to(DEV), bins.to(DEV)]
        full = abi_call(lib, dev_ins, B, F_, D, h, w, dict.fromkeys(OUTPUTS, True))
        for name, r, mine in zip(("cost",) + OUTPUTS, ref, wrapper):
            assert torch.equal(full[name].cpu().view_as(mine), mine), name
            border = torch.ones(h, w, dtype=torch.bool)
            border[2:-2, 2:-2] = False
            assert torch.equal(mine[..., border], r[..., border]), name
        for flags in itertools.product([False, True], repeat=4):
            want = dict(zip(OUTPUTS, flags))
            got = abi_call(lib, dev_ins, B, F_, D, h, w, want)
            assert sorted(got) == sorted(["cost"] + [k for k in OUTPUTS if want[k]])
            for name, t in got.items():
                assert torch.equal(t, full[name]), (name, want)


@both_formulations
def test_non_contiguous_inputs(impl):
    """``current_feats`` in channels_last, ``lookup_feats`` as a permuted view, ``K`` / ``invK`` expanded from one sample: bit
    for bit the results of their contiguous copies"""
    cur, look, poses, K, invK = (t.to(DEV) for t in inputs(2, 2, 23, 41))
    bins = linear(7)
    cur_cl = cur.contiguous(memory_format=torch.channels_last)
    look_view = look.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    K_x, invK_x = K[:1].expand(2, 4, 4), invK[:1].expand(2, 4, 4)
    for t in (cur_cl, look_view, K_x, invK_x):
        assert not t.is_contiguous()
    assert torch.equal(cur_cl, cur) and torch.equal(look_view, look)
    with formulation(impl):
        plain = run_gpu(cur, look, poses, K_x.contiguous(), invK_x.contiguous(), bins)
        strided = run_gpu(cur_cl, look_view, poses, K_x, invK_x, bins)
    assert float(plain[1].mean()) < 1.0
    for a, b in zip(plain, strided):
        assert torch.equal(a, b)
