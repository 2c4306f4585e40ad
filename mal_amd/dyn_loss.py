"""DynamicDepth's warp/loss methods (dynamicdepth/trainer.py:906-975, 1006-1128) as a mixin with upstream's method names,
arguments and dictionary keys, in the manner of ``mal_amd.trainer.MALLossPath``: a DynamicDepth ``Trainer`` inherits them in
place of its own.  Together with ``rigid_warp.warp_dynamic_objects`` and
``networks.DynamicDepthEncoderMatching`` (17) these are the three pieces of a DynamicDepth step the library covers.

What differs from ManyDepth's loss, all on by default upstream (options.py:298-303):
  --zero_img         compute_reprojection_loss zeroes the candidate AND the target at the candidate's holes -- IN PLACE, on
                     ``inputs[("color", 0, 0)]`` itself, so every later evaluation (the second frame, the identity pair, the
                     next scale, the student's pass after the teacher's, the smoothness term at scale 0) meets the union
  --selec_reproj     where one warped frame is a hole the other frame supplies the loss; where both are, the loss is 0
  --no_teacher_warp  the teacher warps and compares the ORIGINAL frames ``("ori_color", f, 0)``, not the ones
                     ``warp_dynamic_objects`` composed

``DynamicDepthLossPath`` needs ``self.opt`` with: height, width, min_depth, max_depth, frame_ids, scales, zero_img,
selec_reproj, no_teacher_warp, train_teacher_only, avg_reprojection, no_ssim (upstream's string 'true'),
disable_automasking, disable_motion_masking, no_matching_augmentation (string), disparity_smoothness, v1_multiscale,
feat_loss.  The warped candidates are always materialised: --selec_reproj and the logs read ``outputs[("color", f, s)]``.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import _lib as L
from . import functional as Fn
from . import loss_utils


def default_options(**kw):
    """the fields above with dynamicdepth/options.py's defaults"""
    o = dict(height=192, width=512, batch_size=12, min_depth=0.1, max_depth=100.0, frame_ids=[0, -1, 1], scales=[0, 1, 2, 3],
             v1_multiscale=False, disable_automasking=False, avg_reprojection=False, no_ssim="false", zero_img=True,
             selec_reproj=True, no_teacher_warp=True, train_teacher_only=False, disable_motion_masking=False,
             no_matching_augmentation="false", disparity_smoothness=1e-3, feat_loss="false")
    o.update(kw)
    return SimpleNamespace(**o)


class DynamicDepthLossPath:
    convention = Fn.MANYDEPTH

    # ---------------------------------------------------------------- options
    def _refuse(self, is_multi=False):
        opt = self.opt
        if getattr(opt, "v1_multiscale", False):
            raise NotImplementedError("opt.v1_multiscale (dynamicdepth/trainer.py:912-913,1016-1017): the hole-aware loss path "
                                      "warps and compares at full resolution only")
        if is_multi and getattr(opt, "feat_loss", "false") == "true":  # upstream reads it in the student's compute_losses only
            raise NotImplementedError("opt.feat_loss == 'true' (dynamicdepth/trainer.py:1123-1125) calls get_feature_metric_loss "
                                      "in the student's compute_losses, which is outside this loss path")

    def _teacher_ori(self, is_multi):
        opt = self.opt
        return (not is_multi) and bool(opt.no_teacher_warp) and not bool(opt.train_teacher_only)

    def _flags(self):
        opt = self.opt
        fl = 0
        if opt.zero_img:
            fl |= L.F_ZERO_IMG
        if opt.selec_reproj:
            fl |= L.F_SELECT
        if opt.avg_reprojection:
            fl |= L.F_AVG
        if opt.no_ssim == "true":
            fl |= L.F_NO_SSIM
        return fl

    # ---------------------------------------------------------------- warp
    def generate_images_pred(self, inputs, outputs, is_multi=False):
        """dynamicdepth/trainer.py:906-954."""
        self._refuse()
        opt = self.opt
        fids = opt.frame_ids[1:]
        which = "ori_color" if self._teacher_ori(is_multi) else "color"
        for scale in opt.scales:
            disp = outputs[("disp", scale)]
            if tuple(disp.shape[-2:]) != (opt.height, opt.width):
                disp = F.interpolate(disp, [opt.height, opt.width], mode="bilinear", align_corners=False)
            Ts = [outputs[("cam_T_cam", 0, f)] for f in fids]
            if is_multi:
                Ts = [t.detach() for t in Ts]  # don't update posenet based on multi frame prediction (:925-927)
            srcs = [inputs[(which, f, 0)] for f in fids]
            cfg = (float(opt.min_depth), float(opt.max_depth), 1e-7, self.convention)
            res = Fn.WarpFn.apply(disp, inputs[("K", 0)], inputs[("inv_K", 0)], cfg, len(fids), *Ts, *srcs)
            outputs[("depth", 0, scale)] = res[0]
            for i, f in enumerate(fids):
                outputs[("sample", f, scale)] = res[1 + i]
                outputs[("color", f, scale)] = res[1 + len(fids) + i]
                if not opt.disable_automasking:
                    outputs[("color_identity", f, scale)] = srcs[i]

    # ---------------------------------------------------------------- small ops
    def compute_reprojection_loss(self, pred, target):
        """dynamicdepth/trainer.py:958-975, one candidate.  Under --zero_img ``target`` is zeroed in place at ``pred``'s holes,
        as upstream does."""
        fl = self._flags() & (L.F_ZERO_IMG | L.F_NO_SSIM)
        r, _ = Fn.HoleReprojFn.apply(pred, target, fl)
        return r

    @staticmethod
    def compute_loss_masks(reprojection_loss, identity_reprojection_loss):
        """dynamicdepth/trainer.py:977-992."""
        return loss_utils.compute_loss_masks(reprojection_loss, identity_reprojection_loss)

    # ---------------------------------------------------------------- losses
    def compute_losses(self, inputs, outputs, is_multi=False, noise=None):
        """dynamicdepth/trainer.py:1006-1128.  ``noise``: None (drawn as ``loss_utils.draw_noise`` does, one (B,1,H,W) draw per
        scale in scale order, as upstream's ``torch.randn``) or a dict / list indexed by scale."""
        self._refuse(is_multi)
        opt = self.opt
        fids = opt.frame_ids[1:]
        flags = self._flags()
        if (flags & L.F_SELECT) and list(fids) != [-1, 1]:
            raise L.MalError("compute_losses: --selec_reproj reads the frames -1 and 1 (dynamicdepth/trainer.py:1059-1060); "
                             "frame_ids is %s" % (opt.frame_ids,))
        which = "ori_color" if self._teacher_ori(is_multi) else "color"
        losses = {}
        total = 0
        for scale in opt.scales:
            disp = outputs[("disp", scale)]
            color = inputs[("color", 0, scale)]
            target = inputs[("color", 0, 0)]
            B, _, H, W = target.shape
            if ("color", fids[0], scale) not in outputs:
                raise L.MalError("compute_losses: warped images missing; call generate_images_pred first")
            cands = [outputs[("color", f, scale)] for f in fids]
            automask = not opt.disable_automasking
            idents = [inputs[(which, f, 0)].detach() for f in fids] if automask else []
            nz = None
            if automask:  # drawn by the teacher AND the student upstream (:1069), whose mask is then overwritten with ones
                nz = noise[scale] if noise is not None else loss_utils.draw_noise((B, 1, H, W), target.device)
            ext = None
            if is_multi:
                ext = torch.ones(B, 1, H, W, dtype=torch.float32, device=target.device)
                if not opt.disable_motion_masking:
                    ext = ext * outputs["consistency_mask"].unsqueeze(1)
                if not opt.no_matching_augmentation == "true":
                    ext = ext * (1 - outputs["augmentation_mask"])
                ext = ext.contiguous()
            reproj, rp_map, wt, holes, ch, _ = Fn.HolePhotoLossFn.apply(target, None if is_multi else nz, ext, flags,
                                                                automask and not is_multi, len(idents), *cands, *idents)
            # what the kernels decided, beside upstream's keys: (n,B,H,W) hole bytes, the candidate that feeds rp, the weight
            outputs[("hole_mask", scale)], outputs[("hole_choice", scale)], outputs[("hole_weight", scale)] = holes, ch, wt
            loss = reproj
            if is_multi:
                multi_depth = outputs[("depth", 0, scale)]
                mono_depth = outputs[("mono_depth", 0, scale)].detach()
                cons, _, ct = Fn.DistilFn.apply(multi_depth, mono_depth, rp_map, rp_map, None, ext, False)
                outputs["consistency_target/{}".format(scale)] = ct
                losses["consistency_loss/{}".format(scale)] = cons
                loss = loss + cons
            losses["reproj_loss/{}".format(scale)] = reproj
            # the colour of scale 0 IS the target, zeroed by now (upstream's get_smooth_loss reads the same memory)
            loss = loss + opt.disparity_smoothness * loss_utils._smooth(disp, color) / (2 ** scale)
            total = total + loss
            losses["loss/{}".format(scale)] = loss
        losses["loss"] = total / len(opt.scales)
        return losses


class LossPath(DynamicDepthLossPath):
    """stand-alone holder of the loss path (what the tests and scripts/bench_dyn_loss.py drive)"""

    def __init__(self, opt):
        self.opt = opt
