"""Golden vectors of the validation metrics (tests/golden/eval_*.npz) from the REFERENCE's own code.

TEST INFRASTRUCTURE ONLY.  Run where the reference checkout exists (it never travels with the tests):

    python -m scripts.gen_golden_eval [path/to/reference]

``manydepth.trainer`` and ``manydepth.evaluate_depth`` cannot be imported without cv2 and the trainer's other module-level
imports, so ``Trainer.val`` (manydepth/trainer.py:836-1064) and ``compute_errors`` (evaluate_depth.py:35-53) are taken
from the reference files with ``ast`` and executed as they stand, with stand-ins for what they reach outside themselves:
``cv2.resize`` is tests/eval_oracle.py's restatement; ``self`` carries ``opt``, ``val_loader``, ``freeze_tp``,
``depth_bin_tracker`` and a ``model.module`` whose networks return recorded disparities; the ground truth is written where
``val`` reads it (``splits/eigen/gt_depths.npz``, ``../repdepth/splits/cityscapes/gt_depths/NNN_depth.npy``) in a
temporary working directory.  ``disp_to_depth``, ``transformation_from_parameters`` and ``compute_depth_errors`` come from
the importable ``manydepth.layers``.  The per-image ratios are read from ``val``'s locals when it returns, and the clamped
predictions from the arguments of its ``compute_errors`` calls.

The inputs are regenerated in the tests from the recorded seeds (tests/eval_oracle.py's generators use plain IEEE
arithmetic); the files hold the seeds, a sha256 of every generated input, and the reference's outputs.
"""
from __future__ import annotations

import ast
import hashlib
import os
import sys
import tempfile
import textwrap
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import eval_oracle as EO  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
EIGEN_SIZES = [(h // 4, w // 4) for h, w in EO.KITTI_GT_SIZES]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def extract(path, name, cls=None):
    """the source of function ``name`` (a method of ``cls`` if given) in ``path``, dedented"""
    src = open(path).read()
    tree = ast.parse(src)
    nodes = tree.body
    if cls is not None:
        nodes = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    fn = next(n for n in nodes if isinstance(n, ast.FunctionDef) and n.name == name)
    return textwrap.dedent(ast.get_source_segment(src, fn))


def eigen_inputs(seed, dtype=np.float64):
    gts = EO.kitti_gt(seed, 8, sizes=EIGEN_SIZES, density=0.12, dtype=dtype)
    disp = EO.disparities(seed + 1, 8, 48, 160)
    mono = EO.disparities(seed + 2, 8, 48, 160)
    return gts, disp, mono


def cityscapes_inputs(seed):
    gts = EO.cityscapes_gt(seed, 2)
    disp = EO.disparities(seed + 1, 2, 192, 512)
    mono = EO.disparities(seed + 2, 2, 192, 512)
    return gts, disp, mono


class _Net:
    def __init__(self, fn):
        self.fn = fn

    def __call__(self, *a, **k):
        return self.fn(*a, **k)


def run_val(ref, ML, gts, disp, mono, split, batch, **opt):
    """Trainer.val of the reference on recorded disparities -> (returned value, ratios, ratios_mono, [(gt, pred, errors)]
    of every compute_errors call in call order)"""
    calls = []
    ns = {"np": np, "torch": torch, "os": os, "disp_to_depth": ML.disp_to_depth,
          "transformation_from_parameters": ML.transformation_from_parameters,
          "cv2": types.SimpleNamespace(resize=lambda img, size: EO.resize_linear(img, size[0], size[1]))}
    exec(extract(os.path.join(ref, "manydepth", "evaluate_depth.py"), "compute_errors"), ns)
    ref_errors = ns["compute_errors"]

    def compute_errors(gt, pred):
        r = ref_errors(gt, pred)
        calls.append((gt.copy(), pred.copy(), np.array(r, np.float64)))
        return r
    ns["compute_errors"] = compute_errors
    exec(extract(os.path.join(ref, "manydepth", "trainer.py"), "val", cls="Trainer"), ns)
    val = ns["val"]

    N, _, h, w = disp.shape
    loader = []
    for b0 in range(0, N, batch):
        n = min(batch, N - b0)
        c = torch.zeros(n, 3, h, w)
        c[0, 0, 0, 0] = b0  # the stand-in networks read which recorded batch this is
        loader.append({("color", 0, 0): c, ("color", -1, 0): torch.zeros(n, 3, h, w),
                       ("K", 2): torch.eye(4).repeat(n, 1, 1), ("inv_K", 2): torch.eye(4).repeat(n, 1, 1)})

    def batch_of(x):
        b0 = int(x[0, 0, 0, 0])
        return slice(b0, b0 + x.shape[0])
    zeros = lambda feats: (torch.zeros(feats[0].shape[0], 2, 1, 3), torch.zeros(feats[0].shape[0], 2, 1, 3))
    module = types.SimpleNamespace(
        need_pose_dec=True, pose_encoder=_Net(lambda x: x), pose=_Net(zeros),
        encoder=_Net(lambda img, *a: (batch_of(img), None, None)),
        depth=_Net(lambda sl: {("disp", 0): torch.from_numpy(disp[sl])}),
        mono_encoder=_Net(batch_of), mono_depth=_Net(lambda sl: {("disp", 0): torch.from_numpy(mono[sl])}))
    o = dict(debug=False, static_camera=False, eval_split=split, zero_cost_volume=True, notadabins=False,
             pred_depth_scale_factor=1.0, disable_median_scaling=False, max_depth=100.0, dataset="kitti", freeze_tp=False)
    o.update(opt)
    self = types.SimpleNamespace(
        opt=types.SimpleNamespace(**o), val_loader=loader, val_frames_to_load=[0, -1], device=torch.device("cpu"),
        freeze_tp=o["freeze_tp"],
        depth_bin_tracker=types.SimpleNamespace(updated=False, min_depth=0.1, max_depth=20.0),
        model=types.SimpleNamespace(module=module))

    captured = {}

    def tracer(frame, event, arg):
        if frame.f_code is val.__code__:
            def local(fr, ev, a):
                if ev == "return":
                    captured.update({k: fr.f_locals.get(k) for k in ("ratios", "ratios_mono")})
                return local
            return local
        return None
    with tempfile.TemporaryDirectory() as tmp:
        work = os.path.join(tmp, "work")
        os.makedirs(os.path.join(work, "splits", "eigen"))
        np.savez(os.path.join(work, "splits", split if split != "cityscapes" else "eigen", "gt_depths.npz"),
                 data=np.array(gts + [None], dtype=object)[:-1])
        cs = os.path.join(tmp, "repdepth", "splits", "cityscapes", "gt_depths")
        os.makedirs(cs)
        if split == "cityscapes":
            for i, g in enumerate(gts):
                np.save(os.path.join(cs, str(i).zfill(3) + "_depth.npy"), g)
        cwd = os.getcwd()
        os.chdir(work)
        sys.settrace(tracer)
        try:
            ret = val(self)
        finally:
            sys.settrace(None)
            os.chdir(cwd)
    return ret, captured.get("ratios"), captured.get("ratios_mono"), calls


def main(ref=None):
    from oracle.gen_golden import REF
    ref = ref or REF
    sys.path.insert(0, ref)
    import manydepth.layers as ML
    from tests.eval_oracle import compute_errors as oracle_errors

    # ---- the errors functions on mixed float32 / float64 inputs
    rng = np.random.default_rng(11)
    z = {"numpy_version": np.array(np.__version__), "torch_version": np.array(torch.__version__)}
    gt64 = 1e-3 + 79.0 * rng.random(3001)
    pr32 = (gt64 * (0.6 + 0.8 * rng.random(3001))).astype(np.float32)
    ns = {"np": np}
    exec(extract(os.path.join(ref, "manydepth", "evaluate_depth.py"), "compute_errors"), ns)
    for tag, g, p in (("f64_f32", gt64, pr32), ("f32_f32", gt64.astype(np.float32), pr32),
                      ("f64_f64", gt64, pr32.astype(np.float64) * 1.0000001), ("f32_f64", gt64.astype(np.float32),
                                                                             pr32.astype(np.float64))):
        z["errors/%s/gt" % tag], z["errors/%s/pred" % tag] = g, p
        r = ns["compute_errors"](g, p)
        z["errors/%s/ref" % tag] = np.array(r, np.float64)
        z["errors/%s/ref_dtypes" % tag] = np.array([str(np.asarray(v).dtype) for v in r])
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(r, oracle_errors(g, p)))
    for tag, g, p in (("f32", gt64.astype(np.float32), pr32), ("f64", gt64, pr32.astype(np.float64))):
        r = ML.compute_depth_errors(torch.from_numpy(g), torch.from_numpy(p))
        z["torch/%s/ref" % tag] = np.array([float(v) for v in r], np.float64)
        z["torch/%s/ref_dtypes" % tag] = np.array([str(v.dtype) for v in r])
    np.savez(os.path.join(OUT, "eval_errors.npz"), **z)

    # ---- eigen: 8 images at quarter KITTI sizes; median scaling with the teacher, and --disable_median_scaling with a
    # scale factor and freeze_tp; float64 and float32 ground truth
    z = {"numpy_version": np.array(np.__version__), "sizes": np.array(EIGEN_SIZES)}
    runs = [("ms_mono_f64", 101, np.float64, dict(freeze_tp=False)),
            ("noms_sf_f64", 101, np.float64, dict(freeze_tp=True, disable_median_scaling=True, pred_depth_scale_factor=5.4)),
            ("sf_mono_f32", 202, np.float32, dict(freeze_tp=False, pred_depth_scale_factor=0.5)),
            ("noms_mono_f64", 303, np.float64, dict(freeze_tp=False, disable_median_scaling=True, max_depth=80.0,
                                                       pred_depth_scale_factor=0.5))]
    for tag, seed, dt, opt in runs:
        gts, disp, mono = eigen_inputs(seed, dt)
        z[tag + "/seed"] = np.array(seed)
        z[tag + "/gt_f64"] = np.array(dt is np.float64)
        z[tag + "/input_sha"] = np.array(digest(*gts, disp, mono))
        z[tag + "/opt"] = np.array(repr(sorted(opt.items())))
        ret, ratios, ratios_mono, calls = run_val(ref, ML, gts, disp, mono, "eigen", 3, **opt)
        store(z, tag + "/", ret, ratios, ratios_mono, calls, not opt["freeze_tp"], True)
    np.savez(os.path.join(OUT, "eval_eigen.npz"), **z)

    # ---- cityscapes: 2 images of 1024x2048 float32 ground truth, regenerated in the tests from the seed
    z = {"numpy_version": np.array(np.__version__)}
    gts, disp, mono = cityscapes_inputs(404)
    z["seed"] = np.array(404)
    z["input_sha"] = np.array(digest(*gts, disp, mono))
    ret, ratios, ratios_mono, calls = run_val(ref, ML, gts, disp, mono, "cityscapes", 2, freeze_tp=False)
    store(z, "", ret, ratios, ratios_mono, calls, True, False)
    np.savez(os.path.join(OUT, "eval_cityscapes.npz"), **z)
    for f in ("eval_errors", "eval_eigen", "eval_cityscapes"):
        print(f, os.path.getsize(os.path.join(OUT, f + ".npz")))


def store(z, prefix, ret, ratios, ratios_mono, calls, mono_flag, full_preds):
    """the returned means, and per image (student, then teacher): compute_errors' arguments reduced to the clamped
    prediction (sha256 + all of it or its head), its valid count, the errors and the ratios"""
    z[prefix + "mean"] = np.asarray(ret[0] if mono_flag else ret, np.float64)
    if mono_flag:
        z[prefix + "mean_mono"] = np.asarray(ret[1], np.float64)
    step = 2 if mono_flag else 1
    for who, off, rat in (("student", 0, ratios), ("mono", 1, ratios_mono)):
        if who == "mono" and not mono_flag:
            continue
        sel = calls[off::step]
        preds = [p for _, p, _ in sel]
        z[prefix + who + "/errors"] = np.array([r for _, _, r in sel])
        z[prefix + who + "/pred_sha"] = np.array([digest(p) for p in preds])
        z[prefix + who + "/n"] = np.array([p.size for p in preds])
        if full_preds:
            z[prefix + who + "/pred"] = np.concatenate(preds)
        else:
            z[prefix + who + "/pred_head"] = np.concatenate([p[:256] for p in preds])
        if rat is not None and len(rat):
            z[prefix + who + "/ratios"] = np.array(rat)


if __name__ == "__main__":
    main(*sys.argv[1:])
