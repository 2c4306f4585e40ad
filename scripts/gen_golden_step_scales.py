"""Golden vectors for the one-call step with --distil and --scales 0 1 2 3 (sclm = 3) from the REFERENCE's own functions.

TEST INFRASTRUCTURE ONLY.  Run where the reference checkout exists (it never travels with the tests):

    python -m scripts.gen_golden_step_scales

``manydepth.trainer`` is not importable even with inert stand-ins for its imports: besides cv2, wandb, accelerate and
torchmetrics it pulls detectron2, mask2former, the never-committed ``manydepth/vis.py`` and its own ``matcher`` at module
level.  So the glue of ``Trainer.generate_images_pred`` (manydepth/trainer.py:1088-1165: per scale, the disparity upsampled
to full resolution, ``BackprojectDepth`` / ``Project3D`` / border ``grid_sample`` of the full-resolution sources, then the
producer; ``self.has_ins`` / ``self.multi_has_ins`` keep the LAST call's answer) and of ``process_batch`` (:573-612) is
restated here, as ``oracle.gen_golden.run_reference_step`` does for one scale; every arithmetic step goes through the
reference's own objects (``SSIM``, ``disp_to_depth``, ``BackprojectDepth``, ``Project3D``, ``compute_mono_losses``,
``compute_main_losses``, ``compute_reprojection_loss``) and ATen.  The producer is the stand-in of the other fixtures
(``mal_amd.synthetic.fake_image_synthesis``: Mask2Former is out of scope).

Recorded: every loss; every leaf gradient, the lower scales' disparities included (no loss reads them: zeros); the
teacher's (and with --main_temporal the student's) ``("color", f, s)`` / ``("syn", f, s)`` for s = 1..3 as sums plus an
8x8-strided subsample (``oracle.gen_golden.summarize``), which keeps each file far below 1 MB.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import OUT, import_reference, multiscale_inputs, pack_inputs, quantize_batch, summarize  # noqa: E402

SCLM = 3


def last_none(synth, last):
    """the stand-in producer, except that its call at scale ``last`` writes nothing and reports no instance"""
    def run(inputs, outputs, scale):
        if scale == last:
            return False
        return synth(inputs, outputs, scale)
    return run


def run_case(ML, MLU, q, opt_kw, noise_seed, tag, producer="fake"):
    from mal_amd.synthetic import to_dicts, fake_image_synthesis
    from oracle.mal_oracle import default_opt

    B, _, H, W = q["color0"].shape
    opt = default_opt(height=H, width=W, batch_size=B, sclm=SCLM, **opt_kw)
    inputs, mono_outputs, outputs, leaves = to_dicts(q, ML.transformation_from_parameters)
    _, low = multiscale_inputs(q, SCLM)
    for name, outs in (("disp_teacher", mono_outputs), ("disp_student", outputs)):
        for s in range(1, SCLM + 1):
            leaf = low[name][s].clone().requires_grad_(True)
            leaves["%s_s%d" % (name, s)] = leaf
            outs[("disp", s)] = leaf
    ssim = ML.SSIM()
    backproject = ML.BackprojectDepth(B, H, W)
    project = ML.Project3D(B, H, W)
    synth = fake_image_synthesis(q["syn_rects"])
    if producer == "lastnone":
        synth = last_none(synth, SCLM)

    def gen_pred(outs, is_multi):  # glue: trainer.py:1088-1165
        has = False
        for scale in range(opt.sclm + 1):
            disp = F.interpolate(outs[("disp", scale)], [H, W], mode="bilinear", align_corners=False)
            _, depth = ML.disp_to_depth(disp, opt.min_depth, opt.max_depth)
            outs[("depth", 0, scale)] = depth
            for f in (-1, 1):
                T = outs[("cam_T_cam", 0, f)]
                if is_multi:
                    T = T.detach()
                pts = backproject(depth, inputs[("inv_K", 0)])
                grid = project(pts, inputs[("K", 0)], T)
                outs[("sample", f, scale)] = grid
                outs[("color", f, scale)] = F.grid_sample(inputs[("color", f, 0)], grid, padding_mode="border",
                                                          align_corners=True)
            if (not is_multi and opt.temporal) or (is_multi and opt.main_temporal):
                has = synth(inputs, outs, scale)  # self.has_ins / self.multi_has_ins: overwritten per scale
        return has

    d = {}
    shape = (B, 1, H, W)
    torch.manual_seed(noise_seed)
    d["in/noise_mono"] = torch.randn(shape).numpy()
    d["in/noise_main"] = torch.randn(shape).numpy()
    d["in/noise_seed"] = np.int64(noise_seed)

    has_ins = gen_pred(mono_outputs, False) and opt.temporal
    torch.manual_seed(noise_seed)
    mono_losses, mono_reproj = MLU.compute_mono_losses(ssim, inputs, mono_outputs, opt.temporal, has_ins)
    for key in list(mono_outputs.keys()):
        if isinstance(key, tuple) and key[0] in ("depth", "disp"):
            outputs[("mono_" + key[0],) + tuple(key[1:])] = mono_outputs[key]
    mono_d = outputs[("mono_depth", 0, 0)]  # trainer.py:1066-1076 / :592-593
    matching = 1 / outputs["lowest_cost"].unsqueeze(1)
    mm = ((matching - mono_d) / mono_d) < 1.0
    mm = mm * (((mono_d - matching) / matching) < 1.0)
    outputs["consistency_mask"] = outputs["consistency_mask"] * mm[:, 0]
    disp_e = (mono_outputs[("disp", 0)].detach() + outputs[("disp", 0)].detach()) / 2.0  # trainer.py:594-600,1172-1207
    disp_e = F.interpolate(disp_e, [H, W], mode="bilinear", align_corners=False)
    _, depth_e = ML.disp_to_depth(disp_e, opt.min_depth, opt.max_depth)
    rr = []
    for f in (-1, 1):
        pts = backproject(depth_e, inputs[("inv_K", 0)])
        grid = project(pts, inputs[("K", 0)], outputs[("cam_T_cam", 0, f)].detach())
        pred = F.grid_sample(inputs[("color", f, 0)], grid, padding_mode="border", align_corners=True)
        rr.append(MLU.compute_reprojection_loss(ssim, pred, inputs[("color", 0, 0)]))
    ensemble_reproj = torch.min(torch.cat(rr, 1), dim=1, keepdim=True)[0]
    multi_has = gen_pred(outputs, True) and opt.main_temporal
    w_list = [0.7, 0.3]
    losses, _, _ = MLU.compute_main_losses(ssim, inputs, outputs, mono_reproj, ensemble_reproj, opt, None, w_list, multi_has)
    for k, v in mono_losses.items():
        losses[k] = losses[k] + v
    losses["loss"].backward()

    d["final_loss"] = np.float64(losses["loss"].item())
    d["has_ins"] = np.int64(bool(has_ins))
    d["multi_has_ins"] = np.int64(bool(multi_has))
    for k, v in mono_losses.items():
        d["mono_losses/" + k] = np.float64(v.item())
    for k, v in losses.items():
        d["losses/" + k] = np.float64(v.item())
    for who, outs, on in (("mono", mono_outputs, opt.temporal), ("multi", outputs, opt.main_temporal)):
        if not on:
            continue
        for s in range(1, SCLM + 1):
            for f in (-1, 1):
                fn = "m1" if f < 0 else "p1"
                summarize("%s/color_%s_s%d" % (who, fn, s), outs[("color", f, s)], d, False)
                if ("syn", f, s) in outs:
                    summarize("%s/syn_%s_s%d" % (who, fn, s), outs[("syn", f, s)], d, False)
    for k, t in leaves.items():
        g = t.grad if t.grad is not None else torch.zeros_like(t)
        d["grad/" + k] = g.numpy()
    d.update(pack_inputs(q))
    for name in ("disp_teacher", "disp_student"):
        for s in range(1, SCLM + 1):
            d["in/%s_s%d" % (name, s)] = low[name][s].half().numpy()
    d["sclm"] = np.int64(SCLM)
    d["producer"] = np.array(producer)
    d["opt"] = np.array(repr(sorted(dict(opt_kw, sclm=SCLM).items())))
    path = os.path.join(OUT, tag + ".npz")
    np.savez_compressed(path, **d)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB", "final_loss", d["final_loss"], "has_ins", bool(has_ins))


def main():
    ML, MLU, _ = import_reference()
    from mal_amd.synthetic import make_batch
    torch.set_num_threads(8)
    q = quantize_batch(make_batch(2, 48, 96, seed=1240, with_syn=True))
    run_case(ML, MLU, q, {"temporal": True}, 1010, "step_b2_48x96_sclm3_temporal")
    run_case(ML, MLU, q, {"temporal": True, "main_temporal": True}, 1011, "step_b2_48x96_sclm3_temporal_main")
    run_case(ML, MLU, q, {"temporal": True}, 1012, "step_b2_48x96_sclm3_lastnone", producer="lastnone")


if __name__ == "__main__":
    main()
