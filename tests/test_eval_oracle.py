"""CPU: the validation-metrics oracle (tests/eval_oracle.py) against the reference's own numbers
(tests/golden/eval_*.npz, scripts/gen_golden_eval.py), the resize restatement's two forms, the crop windows, the
evaluator's ground-truth packing, and the argument checks of the mal_eval_* entry points (no device needed)."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from tests import eval_oracle as EO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EIGEN_SIZES = [(h // 4, w // 4) for h, w in EO.KITTI_GT_SIZES]


def golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def eigen_inputs(seed, gt_f64):
    gts = EO.kitti_gt(seed, 8, sizes=EIGEN_SIZES, density=0.12, dtype=np.float64 if gt_f64 else np.float32)
    return gts, EO.disparities(seed + 1, 8, 48, 160), EO.disparities(seed + 2, 8, 48, 160)


def cityscapes_inputs(seed):
    return EO.cityscapes_gt(seed, 2), EO.disparities(seed + 1, 2, 192, 512), EO.disparities(seed + 2, 2, 192, 512)


def run_opt(opt_text):
    return dict(eval(opt_text))  # a repr of sorted (key, value) pairs written by the generator


def check_run(z, prefix, gts, disp, mono, split, opt):
    mono_flag = not opt.get("freeze_tp", False)
    ms = not opt.get("disable_median_scaling", False)
    sf = opt.get("pred_depth_scale_factor", 1.0)
    max_depth = opt.get("max_depth", 100.0)
    sd = EO.disp_to_depth(disp[:, 0], 1e-3, 80)[0]
    md = EO.disp_to_depth(mono[:, 0], 1e-3, max_depth)[0]
    whos = [("student", sd, ms, sf)] + ([("mono", md, True, None)] if mono_flag else [])
    for who, d, scaled, factor in whos:
        res = [EO.evaluate_image(gts[i], d[i], split, scaled, factor) for i in range(len(gts))]
        assert [r["n"] for r in res] == list(z[prefix + who + "/n"])
        assert [digest(r["pred"]) for r in res] == list(z[prefix + who + "/pred_sha"]), who
        if prefix + who + "/pred" in z:
            assert np.concatenate([r["pred"] for r in res]).tobytes() == z[prefix + who + "/pred"].tobytes()
        if scaled:
            ratios = np.array([r["ratio"] for r in res])
            assert ratios.dtype == z[prefix + who + "/ratios"].dtype
            assert ratios.tobytes() == z[prefix + who + "/ratios"].tobytes(), who
        else:
            assert prefix + who + "/ratios" not in z
        errs = np.array([np.array(r["errors"], np.float64) for r in res])
        assert errs.tobytes() == z[prefix + who + "/errors"].tobytes(), who
        mean = np.array([r["errors"] for r in res]).mean(0)
        key = prefix + ("mean" if who == "student" else "mean_mono")
        assert np.asarray(mean, np.float64).tobytes() == z[key].tobytes(), who


def test_fixture_versions_recorded():
    for name in ("eval_errors", "eval_eigen", "eval_cityscapes"):
        assert str(golden(name)["numpy_version"]).count(".") == 2
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 1 << 20


def test_oracle_reproduces_eigen_fixture():
    z = golden("eval_eigen")
    tags = sorted({k.split("/")[0] for k in z if "/" in k})
    assert len(tags) == 4
    for tag in tags:
        gts, disp, mono = eigen_inputs(int(z[tag + "/seed"]), bool(z[tag + "/gt_f64"]))
        assert digest(*gts, disp, mono) == str(z[tag + "/input_sha"]), "the seeded generators drifted"
        check_run(z, tag + "/", gts, disp, mono, "eigen", run_opt(str(z[tag + "/opt"])))


def test_oracle_reproduces_cityscapes_fixture():
    z = golden("eval_cityscapes")
    gts, disp, mono = cityscapes_inputs(int(z["seed"]))
    assert digest(*gts, disp, mono) == str(z["input_sha"])
    check_run(z, "", gts, disp, mono, "cityscapes", {})


def test_oracle_reproduces_errors_fixture():
    z = golden("eval_errors")
    for tag in ("f64_f32", "f32_f32", "f64_f64", "f32_f64"):
        r = EO.compute_errors(z["errors/%s/gt" % tag], z["errors/%s/pred" % tag])
        assert [str(np.asarray(v).dtype) for v in r] == list(z["errors/%s/ref_dtypes" % tag])
        assert np.array(r, np.float64).tobytes() == z["errors/%s/ref" % tag].tobytes()


def test_resize_pointwise_equals_two_pass():
    rng = np.random.default_rng(5)
    for (sh, sw), (dh, dw) in [((48, 160), (93, 309)), ((192, 640), (375, 1242)), ((7, 9), (5, 4)), ((192, 512), (768, 2048)),
                               ((6, 6), (6, 6)), ((2, 3), (11, 17))]:
        src = rng.random((sh, sw)).astype(np.float32)
        full = EO.resize_linear(src, dw, dh)
        assert full.shape == (dh, dw) and full.dtype == np.float32
        ys, xs = np.nonzero(np.ones((dh, dw), bool))
        assert EO.resize_at(src, dw, dh, ys, xs).tobytes() == full[ys, xs].tobytes()
        assert EO.resize_at(src, dw, dh, ys, xs, True).tobytes() == EO.resize_linear(src, dw, dh, True)[ys, xs].tobytes()
    # same size is the identity; a constant image stays constant along the columns, the clamped rows keep their weight
    src = rng.random((6, 6)).astype(np.float32)
    assert EO.resize_linear(src, 6, 6).tobytes() == src.tobytes()
    assert (EO.resize_linear(np.full((4, 5), 0.3, np.float32), 11, 4)[:, -1] == np.float32(0.3)).all()


def test_eigen_crop_windows_of_kitti_sizes():
    for h, w in EO.KITTI_GT_SIZES + EIGEN_SIZES:
        want = np.array([0.40810811 * h, 0.99189189 * h, 0.03594771 * w, 0.96405229 * w]).astype(np.int32)
        got = EO.eigen_crop(h, w)
        assert got.dtype == np.int32 and got.tolist() == want.tolist()
        assert got.tolist() == [int(0.40810811 * h), int(0.99189189 * h), int(0.03594771 * w), int(0.96405229 * w)]
    assert EO.eigen_crop(375, 1242).tolist() == [153, 371, 44, 1197]


def test_evaluator_packs_what_the_oracle_masks():
    """DepthEvaluator's ground-truth packing (host-side numpy) on device='cpu': valid counts, order, medians"""
    from mal_amd.evaluate import DepthEvaluator
    gts = EO.kitti_gt(3, 4, sizes=EIGEN_SIZES, density=0.1)
    for split in ("eigen", "other"):
        ev = DepthEvaluator(gts, split, device="cpu")
        vals = ev.gt.numpy()
        idx = ev.idx.numpy()
        for i, g in enumerate(gts):
            win, (gh, gw), (ys, xs), mask = EO.valid_points(g, split)
            a, b = ev.offsets[i], ev.offsets[i + 1]
            assert ev.counts[i] == ys.size == b - a
            assert (idx[a:b] == ys * gw + xs).all()
            assert vals[a:b].tobytes() == win[mask].tobytes()
    cs = EO.cityscapes_gt(9, 1, h=1024, w=2048)
    ev = DepthEvaluator(cs, "cityscapes", device="cpu")
    win, _, (ys, xs), mask = EO.valid_points(cs[0], "cityscapes")
    assert ev.counts[0] == mask.sum() and ev.offsets[1] == mask.size
    assert ev.gt.numpy().reshape(mask.shape)[mask].tobytes() == win[mask].tobytes()


def test_evaluator_rejects_bad_ground_truth():
    from mal_amd.evaluate import DepthEvaluator
    gts = EO.kitti_gt(3, 3, sizes=EIGEN_SIZES, density=0.1)
    empty = np.zeros_like(gts[1])
    empty[0, 0] = 5.0  # outside the eigen crop
    with pytest.raises(ValueError, match="image 1 has no valid"):
        DepthEvaluator([gts[0], empty, gts[2]], "eigen", device="cpu")
    with pytest.raises(ValueError, match="float64 or all float32"):
        DepthEvaluator([gts[0], gts[1].astype(np.float32)], "eigen", device="cpu")
    with pytest.raises(ValueError, match="too small"):
        DepthEvaluator([np.ones((100, 100))], "cityscapes", device="cpu")


def test_eval_entry_points_reject_bad_arguments_without_device():
    from mal_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.mal_struct_bytes(5) == C.sizeof(_lib.EvalSeg) and lib.mal_struct_bytes(6) == C.sizeof(_lib.EvalArgs)
    assert lib.mal_eval_accumulate(None) == -1
    fake = 0x1000  # never dereferenced: every check below fails before any HIP call
    good = dict(n_images=4, first=0, B=2, H=8, W=16, gt_f64=1, median_scaling=1, resize_ulp=0, min_depth_disp=1e-3,
                max_depth_disp=80.0, scale_factor=1.0, clamp_min=1e-3, clamp_max=80.0, seg=fake, idx=fake, gt=fake,
                disp=fake, pred=fake, img_out=fake, stream=None)
    bad = [dict(seg=None), dict(gt=None), dict(disp=None), dict(pred=None), dict(img_out=None), dict(n_images=0),
           dict(B=0), dict(first=-1), dict(first=3), dict(B=5), dict(scale_factor=0.0), dict(scale_factor=float("inf")),
           dict(min_depth_disp=0.0), dict(max_depth_disp=1e-4), dict(clamp_min=0.0), dict(clamp_max=1e-4),
           dict(resize_ulp=9)]
    for kw in bad:
        a = _lib.EvalArgs(**dict(good, **kw))
        assert lib.mal_eval_accumulate(C.byref(a)) == -1, kw
    a = _lib.EvalArgs(**dict(good, H=0))
    assert lib.mal_eval_accumulate(C.byref(a)) == -2
    assert lib.mal_eval_mean(None, 4, fake, None) == -1
    assert lib.mal_eval_mean(fake, 0, fake, None) == -1
    assert lib.mal_eval_errors_workspace_bytes(0) == 0
    ws = lib.mal_eval_errors_workspace_bytes(1000)
    assert ws > 0
    assert lib.mal_eval_errors(None, 1, fake, 0, 1000, fake, fake, ws, None) == -1
    assert lib.mal_eval_errors(fake, 1, fake, 0, 0, fake, fake, ws, None) == -1
    assert lib.mal_eval_errors(fake, 1, fake, 0, 1000, fake, fake, ws - 1, None) == -3
