"""GPU: the validation metrics (mal_amd.evaluate, csrc/mal_eval.hip) against the CPU oracle (tests/eval_oracle.py) and the
reference's numbers (tests/golden/eval_*.npz): per-image median ratios bit-equal, a1..a3 counts exact, the other four
metrics within 1e-9 relative (float64 ground truth) / 1e-5 (float32); batch order, grouping and repeated runs give the
same bits; the one-ulp sensitivity of the resize; compute_depth_errors; TrainHarness.val."""
import numpy as np
import pytest
import torch

from tests import eval_oracle as EO
from tests.test_eval_oracle import EIGEN_SIZES, cityscapes_inputs, eigen_inputs, golden, run_opt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


def tol(gt_f64):
    return 1e-9 if gt_f64 else 1e-5


# numpy's float32 log (a SIMD approximation within a few ulp, not correctly rounded: 5 % of float32 inputs differ from
# float32(log(float64(x)))) moves rmse_log of float64 ground truth by up to ~4e-9 relative against the device's correctly
# rounded logf; rmse_log is held at 3e-8 against numpy and at 1e-9 against the oracle with a correctly rounded log.
RMSE_LOG_F64_TOL = 3e-8


def rmse_log_cr(g, p):
    lp = np.log(p.astype(np.float64)).astype(np.float32)
    return np.sqrt(((np.log(g) - lp) ** 2).mean())


def run_gpu(ev, disp, which, batch=12, order=None, **kw):
    """feed raw disparities (N,1,h,w) numpy in batches (in ``order`` of batch starts) -> result(which)"""
    d = torch.from_numpy(disp).to(DEV)
    starts = list(range(0, len(disp), batch))
    for s in (order(starts) if order else starts):
        ev.accumulate(d[s:s + batch], s, which, **kw)
    return ev.result(which)


def check_images(gpu, want_errs, want_ratios, counts, gt_f64, what="", cr=None):
    mean, errs, ratios = gpu
    if want_ratios is None:
        assert ratios is None
    else:
        assert ratios.dtype == np.asarray(want_ratios).dtype, what
        bad = np.nonzero(ratios != want_ratios)[0]
        assert bad.size == 0, "%s: ratios differ at images %s: %r vs %r" % (what, bad[:5], ratios[bad[:5]], want_ratios[bad[:5]])
    # a1..a3: count / n, exact
    got_c = np.rint(errs[:, 4:] * counts[:, None]).astype(np.int64)
    want_c = np.rint(want_errs[:, 4:] * counts[:, None]).astype(np.int64)
    assert (got_c == want_c).all(), "%s: a1..a3 counts differ at images %s" % (what, np.nonzero((got_c != want_c).any(1))[0][:5])
    assert (errs[:, 4:] == want_errs[:, 4:]).all(), what
    t = np.array([tol(gt_f64)] * 3 + [RMSE_LOG_F64_TOL if gt_f64 else tol(gt_f64)])
    w = np.abs(want_errs[:, :4])
    rel = np.abs(errs[:, :4] - want_errs[:, :4]) / np.where(w > 0, w, 1.0)  # exact predictions: 0 must be 0
    assert (rel <= t).all(), "%s: max rel per metric %s" % (what, rel.max(0))
    if cr is not None and gt_f64:
        rel_cr = np.abs(errs[:, 3] - cr) / cr
        assert rel_cr.max() <= 1e-9, "%s: rmse_log vs a correctly rounded logf: %.3e" % (what, rel_cr.max())
    want_mean = np.array(want_errs).mean(0)
    assert (np.abs(mean - want_mean) <= t.max() * np.abs(want_mean)).all(), (what, mean, want_mean)
    return rel.max()


def oracle_set(gts, disp, split, median_scaling, scale_factor, max_depth=80.0, **kw):
    sd = EO.disp_to_depth(disp[:, 0], 1e-3, max_depth)[0]
    res = [EO.evaluate_image(gts[i], sd[i], split, median_scaling, scale_factor, **kw) for i in range(len(gts))]
    errs = np.array([np.array(r["errors"], np.float64) for r in res])
    ratios = np.array([r["ratio"] for r in res]) if median_scaling else None
    oracle_set.cr = np.array([rmse_log_cr(r["gt"], r["pred"]) for r in res])
    return errs, ratios, np.array([r["n"] for r in res]), res


# ---------------------------------------------------------------- the errors functions
def test_compute_errors_matches_reference_fixture():
    from mal_amd.evaluate import compute_errors
    z = golden("eval_errors")
    for tag in ("f64_f32", "f32_f32", "f64_f64", "f32_f64"):
        g, p = z["errors/%s/gt" % tag], z["errors/%s/pred" % tag]
        r = compute_errors(torch.from_numpy(g).to(DEV), torch.from_numpy(p).to(DEV))
        assert [str(v.dtype).replace("torch.", "") for v in r] == list(z["errors/%s/ref_dtypes" % tag]), tag
        got, want = np.array([float(v) for v in r]), z["errors/%s/ref" % tag]
        assert (got[4:] == want[4:]).all(), tag
        t = [1e-5] * 4 if tag == "f32_f32" else [1e-9] * 3 + [RMSE_LOG_F64_TOL]
        assert (np.abs(got[:4] - want[:4]) / want[:4] <= t).all(), (tag, got, want)


def test_compute_depth_errors_matches_torch_reference():
    from mal_amd import layers
    z = golden("eval_errors")
    for tag, (g, p) in (("f32", (z["errors/f32_f32/gt"], z["errors/f32_f32/pred"])),
                        ("f64", (z["errors/f64_f32/gt"], z["errors/f32_f64/pred"]))):
        r = layers.compute_depth_errors(torch.from_numpy(g).to(DEV), torch.from_numpy(p).to(DEV))
        assert [str(v.dtype) for v in r] == list(z["torch/%s/ref_dtypes" % tag]), tag
        assert all(v.dim() == 0 and v.is_cuda for v in r)
        got, want = np.array([float(v) for v in r]), z["torch/%s/ref" % tag]
        assert (np.abs(got - want) / want).max() <= 1e-5, (tag, got, want)


# ---------------------------------------------------------------- the evaluator on the reference's fixtures
def test_evaluator_reproduces_eigen_fixture():
    from mal_amd.evaluate import DepthEvaluator
    z = golden("eval_eigen")
    for tag in sorted({k.split("/")[0] for k in z if "/" in k}):
        opt = run_opt(str(z[tag + "/opt"]))
        gt_f64 = bool(z[tag + "/gt_f64"])
        gts, disp, mono = eigen_inputs(int(z[tag + "/seed"]), gt_f64)
        ev = DepthEvaluator(gts, "eigen", DEV)
        ms = not opt.get("disable_median_scaling", False)
        got = run_gpu(ev, disp, "student", batch=3, median_scaling=ms, scale_factor=opt.get("pred_depth_scale_factor", 1.0))
        check_images(got, z[tag + "/student/errors"], z[tag + "/student/ratios"] if ms else None,
                     z[tag + "/student/n"], gt_f64, tag)
        if not opt.get("freeze_tp", False):
            got = run_gpu(ev, mono, "mono", batch=3, disp_max=opt.get("max_depth", 100.0))
            check_images(got, z[tag + "/mono/errors"], z[tag + "/mono/ratios"], z[tag + "/mono/n"], gt_f64, tag + " mono")


def test_evaluator_reproduces_cityscapes_fixture():
    from mal_amd.evaluate import DepthEvaluator
    z = golden("eval_cityscapes")
    gts, disp, mono = cityscapes_inputs(int(z["seed"]))
    ev = DepthEvaluator(gts, "cityscapes", DEV)
    check_images(run_gpu(ev, disp, "student"), z["student/errors"], z["student/ratios"], z["student/n"], False, "cs")
    check_images(run_gpu(ev, mono, "mono", disp_max=100.0), z["mono/errors"], z["mono/ratios"], z["mono/n"], False, "cs mono")


# ---------------------------------------------------------------- full-size seeded sets against the oracle
def _tile(d, n):
    return np.concatenate([d] * (n // len(d) + 1))[:n]


@pytest.mark.parametrize("gt_f64", [True, False])
def test_eigen_697_full_size(gt_f64):
    from mal_amd.evaluate import DepthEvaluator
    n = 697
    gts = EO.kitti_sparse_gt(7 if gt_f64 else 8, n, dtype=np.float64 if gt_f64 else np.float32)
    disp = _tile(EO.disparities(21, 24, 192, 640), n)
    mono = _tile(EO.disparities(22, 24, 192, 640), n)
    ev = DepthEvaluator(gts, "eigen", DEV)
    errs, ratios, counts, _ = oracle_set(gts, disp, "eigen", True, 1.0)
    check_images(run_gpu(ev, disp, "student"), errs, ratios, counts, gt_f64, "eigen student", oracle_set.cr)
    errs, ratios, counts, _ = oracle_set(gts, mono, "eigen", True, None, max_depth=100.0)
    check_images(run_gpu(ev, mono, "mono", disp_max=100.0), errs, ratios, counts, gt_f64, "eigen mono", oracle_set.cr)
    assert (counts % 2 == 0).any() and (counts % 2 == 1).any()  # both median forms ran


@pytest.mark.parametrize("gt_f64", [False, True])
def test_cityscapes_full_size(gt_f64):
    from mal_amd.evaluate import DepthEvaluator
    gts = [g.astype(np.float64) if gt_f64 else g for g in EO.cityscapes_gt(31, 3)]
    disp = EO.disparities(32, 3, 192, 512)
    ev = DepthEvaluator(gts, "cityscapes", DEV)
    errs, ratios, counts, _ = oracle_set(gts, disp, "cityscapes", True, 1.0)
    check_images(run_gpu(ev, disp, "student", batch=2), errs, ratios, counts, gt_f64, "cityscapes", oracle_set.cr)


def test_odd_even_counts_ties_and_both_clamps():
    """constant and two-valued disparities (every prediction tied at the median), counts of both parities, and
    predictions clamped at 1e-3 and at 80"""
    from mal_amd.evaluate import DepthEvaluator
    sizes = [(40, 120), (41, 121)]
    gts = EO.kitti_gt(41, 6, sizes=sizes, density=0.2)
    gts[0][gts[0] > 0] = 12.5   # ground-truth ties too
    for i, g in enumerate(gts):  # valid counts alternate even, odd
        _, _, (ys, xs), _ = EO.valid_points(g, "other")
        if ys.size % 2 != i % 2:
            g[ys[0], xs[0]] = 0.0
    disp = EO.disparities(42, 6, 24, 64)
    disp[0] = 0.003                                   # one value everywhere
    disp[1, 0, :, :32], disp[1, 0, :, 32:] = 0.002, 0.004   # two plateaus
    disp[2, 0, ::2] = 1.0                             # depth 1e-3: clamped low once scaled below 1
    ev = DepthEvaluator(gts, "other", DEV)
    for ms, sf in ((True, 1.0), (False, 0.5), (False, 30.0)):
        ev.reset()
        errs, ratios, counts, res = oracle_set(gts, disp, "other", ms, sf)
        check_images(run_gpu(ev, disp, "student", batch=4, median_scaling=ms, scale_factor=sf), errs, ratios, counts, True,
                     "ms=%s sf=%s" % (ms, sf))
        if not ms:
            lo = sum(int((r["pred"] == np.float32(1e-3)).sum()) for r in res)
            hi = sum(int((r["pred"] == 80).sum()) for r in res)
            assert (lo > 0) if sf < 1 else (hi > 0), (sf, lo, hi)
    assert set(counts % 2) == {0, 1}


# ---------------------------------------------------------------- determinism, batch order, the one-ulp bound
def test_batch_order_grouping_and_repeat_give_the_same_bits():
    from mal_amd.evaluate import DepthEvaluator
    n = 60
    gts = EO.kitti_sparse_gt(51, n)
    disp = _tile(EO.disparities(52, 8, 192, 640), n)
    ev = DepthEvaluator(gts, "eigen", DEV)
    ref = run_gpu(ev, disp, "student")
    rng = np.random.default_rng(0)
    for kw in (dict(order=lambda s: s[::-1]), dict(order=lambda s: list(rng.permutation(s))), dict(batch=n),
               dict(batch=7), dict()):
        ev.reset()
        got = run_gpu(ev, disp, "student", **kw)
        for a, b in zip(got, ref):
            assert a.tobytes() == b.tobytes(), kw


def test_one_ulp_of_the_resize_bounds_a_cv2_difference():
    """every resized disparity moved by +-1 ulp (what a fused vertical pass or another cv2 build could change): the four
    continuous metrics move by < 1e-6 relative; the a1..a3 decisions that flip are counted per image (oracle) and the
    device path with the nudge still matches the oracle with the same nudge"""
    from mal_amd.evaluate import DepthEvaluator
    n = 48
    gts = EO.kitti_sparse_gt(61, n)
    disp = _tile(EO.disparities(62, 12, 192, 640), n)
    ev = DepthEvaluator(gts, "eigen", DEV)
    base = run_gpu(ev, disp, "student")
    sd = EO.disp_to_depth(disp[:, 0], 1e-3, 80)[0]
    for ulp in (1, -1):
        ev.reset()
        moved = run_gpu(ev, disp, "student", _resize_ulp=ulp)
        errs, ratios, counts, res = oracle_set(gts, disp, "eigen", True, 1.0, ulp=ulp)
        check_images(moved, errs, ratios, counts, True, "ulp %+d" % ulp)
        rel = np.abs(moved[1][:, :4] - base[1][:, :4]) / base[1][:, :4]
        assert rel.max() < 1e-6, (ulp, rel.max(0))
        flips = []
        for i in range(n):
            r0 = EO.evaluate_image(gts[i], sd[i], "eigen", True, 1.0)
            g, p0, p1 = r0["gt"], r0["pred"], res[i]["pred"]
            t0, t1 = np.maximum(g / p0, p0 / g), np.maximum(g / p1, p1 / g)
            flips.append(sum(int(((t0 < c) != (t1 < c)).sum()) for c in (1.25, 1.25 ** 2, 1.25 ** 3)))
        print("ulp %+d: max rel move %s; a1..a3 decisions flipped per image: max %d, mean %.2f of ~%d points"
              % (ulp, ["%.1e" % v for v in rel.max(0)], max(flips), np.mean(flips), counts.mean()))
        assert max(flips) <= 0.01 * counts.min()


# ---------------------------------------------------------------- TrainHarness.val
@pytest.mark.parametrize("freeze_tp", [False, True])
def test_train_harness_val_equals_upstream_order(freeze_tp):
    import random
    from mal_amd import harness
    from mal_amd.evaluate import DepthEvaluator
    from mal_amd.layers import transformation_from_parameters
    torch.manual_seed(0)
    random.seed(0)
    opt = harness.default_options(batch_size=2, height=96, width=160, zero_cost_volume=True, max_depth=100.0)
    h = harness.TrainHarness(opt, DEV)
    h.model.freeze_tp = freeze_tp
    batches = []
    for s in range(3):
        inp = harness.synthetic_inputs(opt, DEV, seed=10 + s)
        batches.append({k: inp[k] for k in (("color", 0, 0), ("color", -1, 0), ("K", 2), ("inv_K", 2))})
    gts = EO.kitti_gt(71, 6, sizes=EIGEN_SIZES, density=0.12)
    out = h.val(batches, DepthEvaluator(gts, "eigen", DEV))
    assert h.model.training
    # the same disparities by calling the model's parts in upstream's order (trainer.py:862-963)
    m = h.model
    m.eval()
    ds, dm = [], []
    lo, hi = h.tracker.compute()
    with torch.no_grad():
        for data in batches:
            feats = [m.pose_encoder(torch.cat([data[("color", -1, 0)], data[("color", 0, 0)]], 1))]
            axisangle, translation = m.pose(feats)
            pose = transformation_from_parameters(axisangle[:, 0], translation[:, 0], invert=True)
            rel = torch.stack([pose], 1) * 0
            output, _, _ = m.encoder(data[("color", 0, 0)], torch.stack([data[("color", -1, 0)]], 1), rel,
                                     data[("K", 2)], data[("inv_K", 2)], min_depth_bin=lo, max_depth_bin=hi)
            ds.append(m.depth(output)[("disp", 0)])
            dm.append(m.mono_depth(m.mono_encoder(data[("color", 0, 0)]))[("disp", 0)])
    m.train()
    ev = DepthEvaluator(gts, "eigen", DEV)
    ev.accumulate(torch.cat(ds), 0, "student")
    want = ev.result("student")[0]
    if freeze_tp:
        assert isinstance(out, np.ndarray) and out.shape == (7,)
        got = out
    else:
        got, got_mono = out
        ev.accumulate(torch.cat(dm), 0, "mono", 1e-3, opt.max_depth)
        assert np.allclose(got_mono, ev.result("mono")[0], rtol=1e-6, atol=0)
    assert np.allclose(got, want, rtol=1e-6, atol=0), (got, want)
    assert np.isfinite(got).all() and 0 < got[0]
