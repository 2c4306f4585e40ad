"""Golden vectors for mal_amd.dyn_loss from the REFERENCE's own ``Trainer.compute_reprojection_loss``,
``Trainer.generate_images_pred`` and ``Trainer.compute_losses`` (dynamicdepth/trainer.py:906-975, 1006-1128).

TEST INFRASTRUCTURE ONLY.  Run in the authoring container only (needs the reference checkout):

    python scripts/gen_golden_dyn_loss.py /path/to/reference

``dynamicdepth/trainer.py`` is loaded BY FILE PATH as ``dynamicdepth.trainer`` inside a stand-in package, with inert stand-ins
for what it imports and these three methods never touch (wandb, tensorboardX, detectron2, the package's rigid_warp, utils,
datasets and networks); ``dynamicdepth/layers.py`` is loaded by path as it is.  The three methods are called UNBOUND on a
namespace that carries what they read from ``self``: the reference's own ``SSIM``, ``BackprojectDepth``, ``Project3D``
objects, ``opt``, ``device``, ``num_scales``.  No arithmetic is restated here.

Per case of ``dyn_loss_restated.GOLDEN_CASES``: the teacher's generate_images_pred + compute_losses, then the student's, on
the SAME ``inputs`` dictionary -- upstream zeroes ``inputs[("color", 0, 0)]`` in place, so the student meets what the
teacher left.  ``torch.randn`` is seeded before each compute_losses and the draws are stored.  tests/dyn_loss_restated.py is
held to the reference BIT FOR BIT here (every loss key, both mutated targets, the warped candidates, hence the hole masks)
before tests/golden/dyn_loss_<case>.npz is written: data only -- the inputs, the noise, every loss key, the target after each
call, the gradients of the leaves.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dyn_loss_restated as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class _Inert(types.ModuleType):
    """a module whose every attribute is an inert callable / sub-module"""

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return _Inert(self.__name__ + "." + k)

    def __call__(self, *a, **kw):
        return None


def import_reference(ref):
    pkg = types.ModuleType("dynamicdepth")
    pkg.__path__ = []  # a package, but nothing is found through it: every sub-module is placed by hand
    names = ["wandb", "tensorboardX", "detectron2", "detectron2.config", "detectron2.projects", "detectron2.projects.deeplab",
             "detectron2.modeling", "detectron2.checkpoint", "dynamicdepth.rigid_warp", "dynamicdepth.utils",
             "dynamicdepth.datasets", "dynamicdepth.networks", "torch_sparse"]
    stand_ins = {n: _Inert(n) for n in names}
    stand_ins["dynamicdepth"] = pkg
    for n in ("rigid_warp", "utils", "datasets", "networks"):
        setattr(pkg, n, stand_ins["dynamicdepth." + n])
    saved = {k: sys.modules.get(k) for k in stand_ins}
    sys.modules.update(stand_ins)
    try:
        layers = _load("dynamicdepth.layers", os.path.join(ref, "dynamicdepth", "layers.py"))
        pkg.layers = layers
        tr = _load("dynamicdepth.trainer", os.path.join(ref, "dynamicdepth", "trainer.py"))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return layers, tr.Trainer


def reference_sequence(c, layers, Trainer):
    opt = R.opt_of(c)
    B, H, W = c["B"], c["H"], c["W"]
    me = types.SimpleNamespace(opt=opt, device="cpu", num_scales=len(opt.scales), ssim=layers.SSIM(),
                               backproject_depth={0: layers.BackprojectDepth(B, H, W)}, project_3d={0: layers.Project3D(B, H, W)},
                               compute_loss_masks=Trainer.compute_loss_masks)
    me.compute_reprojection_loss = lambda pred, target: Trainer.compute_reprojection_loss(me, pred, target)
    inputs = {("color", 0, 0): c["color0"].clone(), ("K", 0): c["K"], ("inv_K", 0): c["inv_K"]}
    for s in opt.scales:
        if s:
            inputs[("color", 0, s)] = c["color0/%d" % s].clone()
    for f, tag in ((-1, "m1"), (1, "p1")):
        inputs[("color", f, 0)] = c["color_" + tag].clone()
        inputs[("ori_color", f, 0)] = c["ori_" + tag].clone()
    lv = {k: c[k].clone().requires_grad_(True) for k in c if k.startswith(("disp_t/", "disp_s/"))}
    lv.update({k: c[k].clone().requires_grad_(True) for k in ("T_m1", "T_p1")})
    res = {}
    outs = {}
    for is_multi, tag in ((False, "t"), (True, "s")):
        outputs = {("cam_T_cam", 0, -1): lv["T_m1"], ("cam_T_cam", 0, 1): lv["T_p1"]}
        for s in opt.scales:
            outputs[("disp", s)] = lv["disp_%s/%d" % (tag, s)]
        if is_multi:
            outputs["consistency_mask"] = c["consistency_mask"].clone()
            outputs["augmentation_mask"] = c["augmentation_mask"].clone()
            for s in opt.scales:
                outputs[("mono_depth", 0, s)] = outs["t"][("depth", 0, s)].detach()
        Trainer.generate_images_pred(me, inputs, outputs, is_multi=is_multi)
        # the draws compute_losses will make, in its order: one (B,1,H,W) per scale
        torch.manual_seed(R.seed_of(c["name"], 17 if is_multi else 3))
        draws = [torch.randn(B, 1, H, W) for _ in opt.scales]
        for s, d in zip(opt.scales, draws):
            assert torch.equal(d, c["noise_%s/%d" % (tag, s)]), "the case's noise is not the seeded draw"
        torch.manual_seed(R.seed_of(c["name"], 17 if is_multi else 3))
        res["losses_" + tag] = Trainer.compute_losses(me, inputs, outputs, is_multi=is_multi)
        res["target_" + tag] = inputs[("color", 0, 0)].clone()
        outs[tag] = outputs
    (res["losses_t"]["loss"] + res["losses_s"]["loss"]).backward()
    res["grads"] = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in lv.items()}
    res["outputs"] = outs
    return res


def bits(t):
    return t.detach().contiguous().numpy().view(np.int32)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    layers, Trainer = import_reference(sys.argv[1])
    torch.set_num_threads(1)
    for name in R.GOLDEN_CASES:
        c = R.golden_case(name)
        opt = R.opt_of(c)
        ref = reference_sequence(c, layers, Trainer)
        mine = R.sequence(c, torch.float32)
        save = {}
        for tag in ("t", "s"):
            for k, v in ref["losses_" + tag].items():
                m = mine["losses_" + tag][k]
                assert np.array_equal(bits(v), bits(m)), "%s: %s of the %s pass is not the reference's bit for bit (%r, %r)" % (
                    name, k, tag, float(v), float(m))
                save["loss_%s:%s" % (tag, k)] = v.detach().numpy()
            assert np.array_equal(bits(ref["target_" + tag]), bits(mine["target_" + tag])), (name, tag, "mutated target")
            save["target_" + tag] = ref["target_" + tag].numpy()
            for s in opt.scales:
                for i, f in enumerate((-1, 1)):
                    w = ref["outputs"][tag][("color", f, s)]
                    assert np.array_equal(bits(w), bits(mine["warped_" + tag][s][1][i])), (name, tag, s, f, "warped candidate")
                    h = (w.detach().sum(1) < 0.1)
                    assert torch.equal(h, mine["recs_" + tag][s]["first"]["holes"][i]), (name, tag, s, f, "hole mask")
                    save["holes_%s/%d/%d" % (tag, s, i)] = h.numpy()
                if tag == "s":
                    ct = ref["outputs"]["s"]["consistency_target/%d" % s]
                    assert np.array_equal(bits(ct), bits(mine["losses_s"]["consistency_target/%d" % s])), (name, s, "consistency_target")
                    save["consistency_target/%d" % s] = ct.detach().numpy()
        for k, g in ref["grads"].items():
            d = float((g - mine["grads"][k]).abs().max())
            assert d <= 1e-6 * max(float(g.abs().max()), 1e-30) + 1e-12, (name, k, d)   # same graph, autograd's own summation order
            save["grad:" + k] = g.numpy()
        # every hole category the default rows are there for, in the teacher's warped pair at scale 0
        cat = R.hole_categories(mine["recs_t"][opt.scales[0]]["first"]["holes"])
        assert min(cat.values()) > 0, (name, cat)
        sums = torch.cat([x.sum(1).flatten() for x in mine["warped_t"][opt.scales[0]][1]])
        assert int(((sums > 0) & (sums < 0.1)).sum()) > 0 and int(((sums >= 0.1) & (sums < 0.2)).sum()) > 0, (name, "soft edge")
        for k, v in c.items():
            if isinstance(v, torch.Tensor):
                save["in:" + k] = v.numpy()
        np.savez_compressed(os.path.join(OUT, "dyn_loss_%s.npz" % name), **save)
        print("case %s: %s, loss_t %.6f loss_s %.6f, target zeroed %d -> %d px" % (
            name, cat, float(ref["losses_t"]["loss"]), float(ref["losses_s"]["loss"]),
            int((ref["target_t"].sum(1) == 0).sum()), int((ref["target_s"].sum(1) == 0).sum())))


if __name__ == "__main__":
    main()
