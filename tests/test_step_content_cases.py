"""The content sweep's case table (tests/step_content_cases.py) on the CPU, with the oracle alone: every case really reaches the
edge it is named after, and the REFERENCE meets the project's gates on it -- everything finite, the fp32 oracle's decisions
against the fp64 oracle's (two correct evaluations) differ at near-ties only, so that a failure of
tests/test_gpu_step_content_sweep.py on the device is the kernels' and not the content's."""
import numpy as np
import pytest
import torch

from tests import hip_harness as HH
from tests import step_content_cases as C
from tests.test_gpu_decisions import _l2rel, _to64, check_decisions_are_near_ties

CASES = [(v, s) for v in C.VARIANTS for s in C.SHAPES]
IDS = ["%s-b%d_%dx%d" % ((v,) + s) for v, s in CASES]
_RUNS = {}


def runs(name, shape):
    """(fp32 oracle, fp64 oracle) of a case: computed once, shared, left unchanged"""
    key = (name, tuple(shape))
    if key not in _RUNS:
        b, n0, n1 = C.case(name, shape)
        _RUNS[key] = (HH.run_oracle(b, {}, n0, n1), HH.run_oracle(C.to64(b), {}, n0.double(), n1.double()))
    return _RUNS[key]


def _rel(a, b):
    return abs(a - b) / abs(b)


def test_the_table():
    assert set(C.VARIANTS) == {"per_sample_K", "large_motion", "behind_camera", "disp_extremes", "flat_images",
                               "dead_weights_one_sample", "dead_weights_all"}
    assert C.SHAPES == ((2, 24, 72), (3, 37, 50)) and C.MS_SHAPE == (3, 40, 72) and C.DR_SHAPE == (2, 40, 72)
    b0, n0, _ = C.case("per_sample_K", C.SHAPES[0])
    b1, n1, _ = C.case("per_sample_K", C.SHAPES[0])
    assert b0 is b1 and n0 is n1                                     # built once
    assert not torch.equal(n0, C.case("large_motion", C.SHAPES[0])[1])  # a generator of its own per case
    from mal_amd.synthetic import make_batch
    ref = make_batch(2, 24, 72, seed=C.seed_of("per_sample_K", (2, 24, 72)))
    assert set(ref) == set(b0) and all(b0[k].shape == v.shape and b0[k].dtype == v.dtype for k, v in ref.items())


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "b%d_%dx%d" % s)
def test_the_masks_of_the_base_batch_bite(shape):
    """augmentation off, and neither mask all-true or all-false in any sample: the student's weight is a proper subset"""
    b, n0, n1 = C.case("base", shape)
    o64 = runs("base", shape)[1]
    N = shape[1] * shape[2]
    assert float(b["augmentation_mask"].abs().sum()) == 0
    cons = b["consistency_mask"].reshape(shape[0], -1).sum(1).numpy()
    w = C.student_weight_sums(o64)
    assert ((0 < w) & (w < cons) & (cons < N)).all(), (w, cons, N)


@pytest.mark.parametrize("name,shape", CASES, ids=IDS)
def test_the_edge_is_really_hit(name, shape):
    b, n0, n1 = C.case(name, shape)
    o32, o = runs(name, shape)
    B, H, W = shape
    N = B * H * W
    b64 = C.to64(b)
    info = {}
    if name in ("per_sample_K", "large_motion"):
        K = b["K"].numpy()
        for i in range(B):
            for j in range(i + 1, B):
                assert all(K[i][r, c] != K[j][r, c] for r, c in ((0, 0), (1, 1), (0, 2), (1, 2))), (i, j)
        assert np.abs(np.einsum("bij,bjk->bik", b["K"].double().numpy(), b["inv_K"].double().numpy())[:, :3, :3] - np.eye(3)).max() <= 1e-5  # inv_K is cast to fp32: entries up to 72 x 2**-24
    if name == "per_sample_K":
        ctrl = HH.run_oracle(C.to64(C.broadcast_K0(b)), {}, n0.double(), n1.double())
        info["loss moves with K[0] broadcast (rel)"] = _rel(ctrl["final"], o["final"])
        assert _rel(ctrl["final"], o["final"]) > 1e-3, (ctrl["final"], o["final"])
    if name == "large_motion":
        for who in ("mono_sample", "multi_sample"):
            share = C.clipped_share(o[who])
            info["clipped share " + who] = share
            assert all(0.25 <= v <= 0.75 for v in share.values()), (who, share)
    if name == "behind_camera":
        z = {who: C.projected_z(b64, who).numpy() for who in ("teacher", "student")}
        for who, v in z.items():
            info["share z' < 0, " + who] = float((v < 0).any(1).mean())
            info["min |z'|, " + who] = float(np.abs(v).min())
            assert (v < 0).any(1).mean() >= 0.10 and np.abs(v).min() >= 1e-3, (who, info)
        # ... and in fp32, what the kernels see
        assert all(np.abs(C.projected_z(b, who).numpy()).min() >= 1e-3 for who in z)
    if name == "disp_extremes":
        ends = [float(v) for v in C.O.disp_to_depth(torch.tensor([1.0, 0.0], dtype=torch.float64), C.MIN_DEPTH, C.MAX_DEPTH)[1]]
        assert abs(ends[0] - C.MIN_DEPTH) <= 1e-12 and abs(ends[1] - C.MAX_DEPTH) <= 1e-9
        for k in ("mono_depth", "multi_depth"):
            assert o[k].min() == ends[0] and o[k].max() == ends[1], (k, o[k].min(), o[k].max())
            info["pixels at the bounds, " + k] = (int((o[k] == ends[0]).sum()), int((o[k] == ends[1]).sum()))
        for k in ("disp_teacher", "disp_student"):  # zero first differences inside the plateaus
            sx, sy = HH._smooth_signs(b64[k])
            assert (sx == 0).sum() > 0 and (sy == 0).sum() > 0
    if name == "flat_images":
        tgt = b64["color0"]
        zero_ssim = zero_l1 = 0
        for p in o["mono_preds"] + o["multi_preds"]:
            p = torch.from_numpy(p)
            zero_ssim += int((C.ssim_preclamp(p, tgt) == 0).sum())
            zero_l1 += int((torch.sign(p - tgt) == 0).sum())
        info["pre-clamp SSIM terms exactly 0"], info["L1 signs exactly 0"] = zero_ssim, zero_l1
        assert zero_ssim >= H * W and zero_l1 >= H * W, info  # sample 0 at least
    if name in C.DEAD:
        base64 = runs("base", shape)[1]
        w = C.student_weight_sums(o)
        info["student weight per sample"] = w.tolist()
        assert float(b["augmentation_mask"].abs().sum()) == 0
        assert _rel(o["final"], base64["final"]) > 1e-3                      # the total moves ...
        for k, v in base64["mono_losses"].items():                          # ... the teacher's own terms do not: no weight of the
            assert o["mono_losses"][k] == v, k                              # student's reaches them
        if name == "dead_weights_one_sample":
            assert w[0] == 0 and w[-1] == 0 and (B == 2 or (w[1:-1] > 0).all()), w
        else:
            assert (w == 0).all(), w
            # 0 / (0 + 1e-7) and the distillation term's weight: exactly zero, not small
            assert o["losses"]["distil_loss"] == 0.0
            assert o["losses"]["reproj_loss/0"] == o["mono_losses"]["reproj_loss/0"]
            # the student's disparity still collects the consistency term (its weight is 1 - 0) and its smoothness term: the
            # oracle's gradient IS the gradient of those two alone, and is not zero
            d = b64["disp_student"].clone().requires_grad_(True)
            _, depth = C.O.disp_to_depth(d, C.MIN_DEPTH, C.MAX_DEPTH)
            rest = (depth - torch.from_numpy(o["mono_depth"])).abs().mean() + 1e-3 * C.O.normalized_smooth_loss(d, b64["color0"])
            rest.backward()
            assert np.abs(o["grads"]["disp_student"]).max() > 0
            assert np.abs(o["grads"]["disp_student"] - d.grad.numpy()).max() <= 1e-12 * np.abs(d.grad.numpy()).max()
    print("content sweep, edge of %s at %s: %s" % (name, shape, info))


@pytest.mark.parametrize("name,shape", CASES, ids=IDS)
def test_the_reference_alone_meets_the_gates(name, shape):
    """fp32 oracle against fp64 oracle as two correct evaluations.  Non-smoothness kinds: the gate as it stands (at most
    3e-4 N + 8 differing pixels per kind, none away from a near-tie).  Smoothness kinds: the second clause only -- the fp64
    oracle normalises before it differences and so do both sides here, the kernels do not; the count of THIS stand-in exceeds
    the cap with plain make_batch content too (11 against 9.7 at 37x50)."""
    b, n0, n1 = C.case(name, shape)
    o32, o64 = runs(name, shape)
    B, H, W = shape
    N = B * H * W
    for o in (o32, o64):
        assert np.isfinite(o["final"]) and all(np.isfinite(v) for v in o["losses"].values())
        assert all(np.isfinite(g).all() for g in o["grads"].values())
        assert all(np.isfinite(o[k]).all() for k in ("mono_reproj", "ens", "multi_cands", "mono_cands", "mono_depth", "multi_depth"))
    d32, d64 = HH.oracle_decisions(o32, b, n0), HH.oracle_decisions(o64, C.to64(b), n0.double())
    diff = HH.decision_differences(d32, d64)
    smooth = {k: diff[k] for k in ("smooth_t", "smooth_s")}
    for k in smooth:
        diff[k] = np.zeros_like(diff[k])
    counts = check_decisions_are_near_ties(diff, o32, b, n0, N)
    for k, name_ in (("smooth_t", "disp_teacher"), ("smooth_s", "disp_student")):
        counts[k] = int(smooth[k].sum())
        assert not (smooth[k] & ~HH.smooth_sign_ambiguous(b[name_].numpy())).any(), k
    # what the device's smoothness kinds WILL be compared on: the kernels take the signs of the raw differences (exact in fp32, a
    # function of the input alone), the fp32 oracle those of the normalised maps -- the gate as it stands, count cap included
    for k, name_ in (("raw smooth_t", "disp_teacher"), ("raw smooth_s", "disp_student")):
        (ax, ay), (bx, by) = HH._raw_smooth_signs(b[name_]), HH._smooth_signs(b[name_])
        m = torch.zeros(b[name_].shape, dtype=torch.bool)
        m[..., :, :-1] |= ax != bx
        m[..., :-1, :] |= ay != by
        counts[k] = int(m.sum())
        assert counts[k] <= 3e-4 * N + 8, (k, counts[k])
        assert not (m.numpy() & ~HH.smooth_sign_ambiguous(b[name_].numpy())).any(), k
    # the floor of the gradient gates: the fp32 forced oracle against the fp64 one, same (fp32) decisions on both sides
    f32 = HH.run_oracle(b, {}, n0, n1, forced=d32)
    f64 = HH.run_oracle(C.to64(b), {}, n0.double(), n1.double(), forced=_to64(d32))
    floors = {k: _l2rel(f32["grads"][k], f64["grads"][k]) for k in HH.LEAVES}
    print("content sweep, reference of %s at %s: differing decisions %s; fp32 forced oracle, L2 rel to fp64: %s"
          % (name, shape, {k: v for k, v in counts.items() if v}, {k: "%.1e" % v for k, v in floors.items()}))
    assert all(np.isfinite(v) for v in floors.values())
    assert {k for k, v in floors.items() if v > 8e-5} == set(C.FLOOR_LEAVES.get((name, tuple(shape)), ())), floors


def test_why_the_flat_half_of_sample_1_is_zero_and_not_one():
    """a bilinear warp of the constant 1.0 is the rounded sum of four rounded weights: some flat pixels come out one ulp below
    1.0 in fp32, their two candidates (0 in exact arithmetic) then tie or not as the weights round, and the winner is a matter
    of rounding at more pixels than the gate's count cap allows.  Zeros warp to zeros exactly."""
    from mal_amd.synthetic import make_batch
    shape = C.SHAPES[0]
    B, H, W = shape
    for value, exact in ((1.0, False), (0.0, True)):
        g = C._gen("flat_images", shape)
        b = C.flat_images(make_batch(B, H, W, seed=C.seed_of("flat_images", shape)), g, value=value)
        n0, n1 = torch.randn(B, 1, H, W, generator=g), torch.randn(B, 1, H, W, generator=g)
        o32 = HH.run_oracle(b, {}, n0, n1)
        inner = np.stack(o32["mono_preds"])[:, 1, :, 2:-2, 2:W // 2 - 8]  # well inside the flat half at these motions
        src = np.stack([b["color_m1"].numpy(), b["color_p1"].numpy()])[:, 1, :, 2:-2, 2:W // 2 - 8]
        assert (src == value).all()
        off = (inner != value) & (np.abs(inner - value) <= 2.0 ** -22)  # a rounding apart (a tap in the texture is further off)
        assert off.any() != exact, (value, int(off.sum()))


def test_the_other_steps_shapes_meet_the_geometry_conditions():
    """the four-scale and the DualRefine step take the three geometry variants at shapes of their own: the conditions on the
    content (not on any loss) hold there too"""
    for shape in (C.MS_SHAPE, C.DR_SHAPE):
        b, _, _ = C.case("per_sample_K", shape)
        assert len({tuple(k.flatten().tolist()) for k in b["K"]}) == shape[0]
        b, _, _ = C.case("behind_camera" if shape == C.DR_SHAPE else "behind_camera_whole_samples", shape)
        for who in ("teacher", "student"):
            for s in range(1 if shape == C.DR_SHAPE else C.MS_SCLM + 1):  # every scale's map as the four-scale step warps with it
                b64 = C.to64(b)
                b64["disp_" + who] = torch.nn.functional.interpolate(HH._lowres(b64, "disp_" + who, s), shape[1:], mode="bilinear",
                                                                     align_corners=False)
                for dt in (b64, {k: (v.float() if torch.is_tensor(v) else v) for k, v in b64.items()}):
                    z = C.projected_z(dt, who).numpy()
                    assert (z < 0).any(1).mean() >= 0.10 and np.abs(z).min() >= 1e-3, (shape, who, s, np.abs(z).min())
        b, _, _ = C.case("large_motion", shape)
        b64 = C.to64(b)
        for who in ("teacher", "student"):
            _, depth = C.O.disp_to_depth(b64["disp_" + who], C.MIN_DEPTH, C.MAX_DEPTH)
            pts = C.O.backproject_depth(depth, b64["inv_K"])
            sample = {}
            for f, s, inv in ((-1, "m1", True), (1, "p1", False)):
                T = C.O.transformation_from_parameters(b64["axisangle_" + s], b64["translation_" + s], inv)
                sample[f] = C.O.project_3d(pts, b64["K"], T, shape[1], shape[2]).numpy()
            share = C.clipped_share(sample)
            assert all(0.25 <= v <= 0.75 for v in share.values()), (shape, who, share)
