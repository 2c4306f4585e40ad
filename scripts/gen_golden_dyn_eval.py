"""Golden vectors for mal_amd.dyn_eval from the REFERENCE's own ``Trainer.compute_depth_losses`` and ``Trainer.val``
(dynamicdepth/trainer.py:1158-1257, :756-905).

TEST INFRASTRUCTURE ONLY.  Run in the authoring container only (needs the reference checkout):

    python scripts/gen_golden_dyn_eval.py /path/to/reference

``dynamicdepth/trainer.py`` is loaded BY FILE PATH inside the stand-in package scripts/gen_golden_dyn_loss.py builds.  Per case
of ``dyn_eval_restated.GOLDEN_CASES``:

  * ``Trainer.compute_depth_losses`` is called UNBOUND on a namespace (opt, gt_depths, depth_metric_names), once per image with
    fresh dictionaries (the per-image metrics) and once more over all images into shared ones (the sums and counts);
  * ``Trainer.val`` is called unbound too, so that its tail (:881-905) runs as written: the loader yields one image per batch,
    opt.no_warp skips the warp block, and the four networks are stand-ins that hand out the case's stored disparities.

The generator runs on the CPU: ``Tensor.cuda`` is made the IDENTITY for the run (upstream calls ``.cuda()`` on the ground truth
and the mask, :1216-1217).  The function's locals (the clamped prediction, the masks, the medians) are read through recording
proxies put in place of the names ``torch`` and ``F`` in the trainer module's globals; they forward every call unchanged.  No
arithmetic is restated here.  tests/dyn_eval_restated.py is held to all of it BIT FOR BIT before
tests/golden/dyn_eval_<case>.npz is written: data only.  The full-size prediction is stored for the student's first image where it
has at most 1000 pixels (the 12x20 case; float32 noise does not compress); at the valid points it is stored for every image and
both networks.
"""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from tests import dyn_eval_restated as R  # noqa: E402
from gen_golden_dyn_loss import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FULL_LIMIT = 1000


class Recording:
    """stands for a module: forwards everything, keeps what the named functions returned (and from_numpy's arguments)"""

    def __init__(self, module, names, log):
        self._module, self._names, self._log = module, names, log

    def __getattr__(self, k):
        v = getattr(self._module, k)
        if k not in self._names:
            return v

        def call(*a, **kw):
            out = v(*a, **kw)
            self._log.append((k, out.detach().clone()))
            return out
        return call


def namespace(c, Trainer, tmp):
    city = c["split"] == "cityscapes"
    opt = types.SimpleNamespace(min_depth=c["min_depth"], max_depth=c["max_depth"], eval_split=c["split"],
                                split="cityscapes_preprocessed" if city else "eigen_zhou", export=False, no_warp=True,
                                dataset="kitti", cv_min="true", cv_set_1=False, cv_pool=False, cv_pool_radius=1, cv_pool_th=0.5)
    if city:
        for i, g in enumerate(c["gt"]):
            np.save(os.path.join(tmp, str(i).zfill(3) + "_depth.npy"), g)
    me = types.SimpleNamespace(opt=opt, gt_depths=tmp if city else c["gt"], depth_metric_names=["de/" + m for m in R.METRICS])
    me.compute_depth_losses = lambda *a, **kw: Trainer.compute_depth_losses(me, *a, **kw)
    return me


def fresh(me):
    d = {}
    for m in me.depth_metric_names:
        d[m] = 0.0
        d["doj/" + m] = 0.0
    d.update({"doj/count": 0.0, "dojpxs": 0, "allpxs": 0})
    return d


def one_image(c, me, i, losses, losses_mono):
    inputs = {"doj_mask": c["doj_mask"][i:i + 1].clone()}
    outputs = {("disp", 0): c["disp"][i:i + 1].clone(), ("mono_disp", 0): c["mono_disp"][i:i + 1].clone()}
    me.compute_depth_losses(inputs, outputs, losses, losses_mono, i, True, accumulate=True)
    return inputs


def run_val(c, me, Trainer):
    """Trainer.val as written, on stand-in networks that hand out the case's disparities"""
    n = len(c["gt"])
    batch = lambda x: int(x.flatten()[0])  # noqa: E731  the image index travels in the colour tensor
    me.set_eval = lambda: None
    me.device = "cpu"
    me.predict_poses = lambda *a, **kw: {}
    me.matching_ids = [0, -1]
    me.min_depth_tracker = me.max_depth_tracker = None
    me.models = {"mono_encoder": batch, "mono_depth": lambda i: {("disp", 0): c["mono_disp"][i:i + 1].clone()},
                 "encoder": lambda x, *a, **kw: (batch(x), None, None), "depth": lambda i: {("disp", 0): c["disp"][i:i + 1].clone()}}
    tag = lambda i: torch.full((1, 1, 1, 1), float(i))  # noqa: E731
    me.val_loader = [{("relative_pose", -1): torch.eye(4)[None], ("color_aug", -1, 0): tag(i), ("color_aug", 0, 0): tag(i),
                      ("K", 2): torch.eye(4)[None], ("inv_K", 2): torch.eye(4)[None], "doj_mask": c["doj_mask"][i:i + 1].clone()}
                     for i in range(n)]
    return Trainer.val(me, mono_eval=True)


def f64(xs):
    return np.array([float(x) for x in xs], np.float64)   # float32 values widen exactly


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.int64 if np.asarray(a).dtype.itemsize == 8 else np.int32),
                          np.asarray(b).view(np.int64 if np.asarray(b).dtype.itemsize == 8 else np.int32))


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    _, Trainer = import_reference(sys.argv[1])
    torch.set_num_threads(1)
    g = Trainer.compute_depth_losses.__globals__
    log = []
    saved = (g["torch"], g["F"], torch.Tensor.cuda)
    g["torch"] = Recording(torch, ("clamp", "median", "from_numpy"), log)
    g["F"] = Recording(F, ("interpolate",), log)
    torch.Tensor.cuda = lambda self, *a, **kw: self
    try:
        for name in R.GOLDEN_CASES:
            c = R.make_case(name, R.GOLDEN_CASES)
            n = len(c["gt"])
            with tempfile.TemporaryDirectory() as tmp:
                me = namespace(c, Trainer, tmp)
                total, total_mono = fresh(me), fresh(me)
                save = {"name": np.array(name), "eval_split": np.array(c["split"]), "n_images": np.array(n),
                        "min_depth": np.array(c["min_depth"]), "max_depth": np.array(c["max_depth"]),
                        "in:disp": c["disp"].numpy(), "in:mono_disp": c["mono_disp"].numpy(), "in:doj_mask": c["doj_mask"].numpy()}
                mine = {w: R.evaluate_case(c, w) for w in ("student", "mono")}
                n_all, n_doj = [], []
                for i in range(n):
                    save["in:gt/%d" % i] = c["gt"][i]
                    del log[:]
                    losses, losses_mono = fresh(me), fresh(me)
                    inputs = one_image(c, me, i, losses, losses_mono)
                    one_image(c, me, i, total, total_mono)
                    clamps = [t for k, t in log if k == "clamp"][:4]
                    medians = [t for k, t in log if k == "median"][:4]
                    mask = [t for k, t in log if k == "from_numpy"][1]
                    y0, x0 = R.valid_points(c["gt"][i], c["split"])[3]
                    doj = mask & inputs["doj_mask"].bool()
                    assert int(doj.sum()) == int(losses["dojpxs"]) and int(mask.sum()) == int(losses["allpxs"])
                    n_all.append(int(mask.sum()))
                    n_doj.append(int(doj.sum()))
                    save["mask/%d" % i], save["doj_mask/%d" % i] = mask.numpy(), doj.numpy()
                    for w, who in enumerate(("student", "mono")):
                        r = mine[who][i]
                        full = clamps[w][0, 0]
                        win = full[y0:y0 + mask.shape[0], x0:x0 + mask.shape[1]]
                        ratio = medians[2 * w] / medians[2 * w + 1]
                        d = losses if who == "student" else losses_mono
                        errs = f64(d[m] for m in me.depth_metric_names)
                        assert same(win[mask].numpy(), r["pred_first"].numpy()), (name, i, who, "first clamp")
                        assert same(clamps[2 + w][mask].numpy(), r["pred"].numpy()), (name, i, who, "scaled prediction")
                        assert same(ratio.numpy(), r["ratio"].numpy()) and ratio.dtype == r["ratio"].dtype, (name, i, who, "ratio")
                        assert same(medians[2 * w + 1].numpy(), r["median"].numpy()), (name, i, who, "median")
                        assert torch.equal(mask, r["mask"]) and torch.equal(doj, r["doj_mask"]), (name, i, "masks")
                        assert same(errs, f64(r["errors"])), (name, i, who, errs, f64(r["errors"]))
                        save["pred_pts/%s/%d" % (who, i)] = win[mask].numpy()
                        save["scaled_pts/%s/%d" % (who, i)] = clamps[2 + w][mask].numpy()
                        save["ratio/%s/%d" % (who, i)] = ratio.numpy()
                        save["median/%s/%d" % (who, i)] = medians[2 * w + 1].numpy()
                        save["errors/%s/%d" % (who, i)] = errs
                        if n_doj[-1] > 0:
                            derrs = f64(d["doj/" + m] for m in me.depth_metric_names)
                            assert same(derrs, f64(r["doj_errors"])), (name, i, who, "doj errors")
                            save["doj_errors/%s/%d" % (who, i)] = derrs
                        if who == "student" and i == 0 and full.numel() <= FULL_LIMIT:
                            assert same(full.numpy(), r["pred_full"].numpy())
                            save["pred_full/student/%d" % i] = full.numpy()
                errors, mono_err, doj_err = run_val(c, me, Trainer)
            assert 0 in n_doj and max(n_doj) > 0, (name, n_doj)   # doj/count differs from the image count
            assert total["doj/count"] == sum(x > 0 for x in n_doj) < n
            agg = {w: R.aggregate(mine[w]) for w in ("student", "mono")}
            for lst, w, pre in ((errors, "student", ""), (mono_err, "mono", ""), (doj_err, "student", "doj/")):
                for m, v in zip(R.METRICS, lst):
                    ref = float(v)
                    assert abs(ref - agg[w][pre + m]) <= 1e-6 * abs(ref), (name, w, pre + m, ref, agg[w][pre + m])  # float32 accumulator of a1..a3
            save["val/errors"], save["val/mono_err"], save["val/doj_err"] = f64(errors), f64(mono_err), f64(doj_err)
            save["val/doj_count"], save["val/dojpxs"], save["val/allpxs"] = (np.array(total["doj/count"]), np.array(int(total["dojpxs"])),
                                                                            np.array(int(total["allpxs"])))
            save["n_all"], save["n_doj"] = np.array(n_all), np.array(n_doj)
            assert R.admissible(c), name
            path = os.path.join(OUT, "dyn_eval_%s.npz" % name)
            np.savez_compressed(path, **save)
            print("case %s: n_all %s n_doj %s, abs_rel %.6f doj/abs_rel %.6f, %d bytes" % (
                name, n_all, n_doj, float(errors[0]), float(doj_err[0]), os.path.getsize(path)))
    finally:
        g["torch"], g["F"], torch.Tensor.cuda = saved


if __name__ == "__main__":
    main()
