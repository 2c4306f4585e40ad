"""DynamicDepth's validation on the device: ``Trainer.compute_depth_losses`` (dynamicdepth/trainer.py:1158-1257) with
``layers.compute_depth_errors`` (dynamicdepth/layers.py:244-262) and the aggregation of ``Trainer.val`` (:881-905), in
libmal_hip.so (csrc/mal_dyn_eval.hip).

It is the number DynamicDepth is judged by: the seven depth errors over the whole image and over the **dynamic-object
region** (``doj/abs_rel`` .. ``doj/a3``), for the student and for the teacher.  ``mal_amd.evaluate.DepthEvaluator`` is MAL's
``val`` and differs from this rule in every step (the disparity is resized there, the depth here; ``np.median`` there,
``torch.median``'s lower middle value here; one region there, two here), so this evaluator stands beside it.

``DynamicDepthEvaluator`` packs a split's ground truth once with ``evaluate.pack_ground_truth``, then takes disparities and
object masks batch by batch -- any batch size; upstream can only do one image at a time -- on the caller's stream with no host
synchronisation.  The results do not depend on the order or grouping of the batches.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .evaluate import METRICS, _planes, _SplitEvaluator, pack_ground_truth

__all__ = ["DynamicDepthEvaluator", "DynamicDepthValPath", "METRICS"]

_MAX_POINTS = 1 << 24   # a1..a3 are float32 means of 0/1: exact below 2^24 points per image


class DynamicDepthEvaluator(_SplitEvaluator):
    """The per-image rule of ``compute_depth_losses`` and ``val``'s aggregation for one split.

    ``gt_depths``: the split's ground truth, a list of 2-D numpy arrays, all float64 or all float32.  ``eval_split``: "eigen"
    or "eigen_benchmark" (depth mask and the crop of :1207-1211) or "cityscapes" (the top round(0.75 H) rows, then the
    [256:, 192:1856] window, depth mask); upstream leaves ``mask`` undefined for any other name, which raises here.
    ``min_depth`` / ``max_depth``: the 1e-3 and 80 upstream has as literals for the ground-truth mask and both clamps.
    An image without a valid pixel raises ValueError (upstream's medians of an empty slice fail); so does one with 2^24 or more.
    """
    ROW = _lib.EVAL_DYN_ROW

    def __init__(self, gt_depths, eval_split, device="cuda", min_depth=1e-3, max_depth=80):
        if eval_split not in ("eigen", "eigen_benchmark", "cityscapes"):
            raise ValueError("DynamicDepthEvaluator: eval_split %r: upstream defines the mask for 'eigen', 'eigen_benchmark' and "
                             "'cityscapes' only (dynamicdepth/trainer.py:1205-1214)" % (eval_split,))
        if (float(min_depth), float(max_depth)) != (1e-3, 80.0):
            raise ValueError("DynamicDepthEvaluator: upstream's 1e-3 and 80 are literals (trainer.py:1164-1165, :1189, :1220); the "
                             "kernels clamp to them")
        self.split, self.device = eval_split, torch.device(device)
        pk = pack_ground_truth(gt_depths, "eigen" if eval_split == "eigen_benchmark" else eval_split, min_depth, max_depth,
                               median="lower")   # torch.median: the lower middle value
        for i, n in enumerate(pk.counts):
            if n >= _MAX_POINTS:
                raise ValueError("DynamicDepthEvaluator: image %d has %d valid points; the float32 means a1..a3 are exact below "
                                 "%d only" % (i, n, _MAX_POINTS))
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise _lib.MalError("DynamicDepthEvaluator: needs a HIP device (there is no CPU path), got %r" % (device,))
        self._upload(pk)

    def accumulate(self, disp, doj_mask, first_index, which="student", disp_min=0.1, disp_max=100.0, export=False):
        """One batch: ``disp`` (B,1,h,w) or (B,h,w) float32 sigmoid outputs (``outputs[("disp", 0)]``, or ``("mono_disp", 0)``
        with which="mono") and ``doj_mask`` (B,1,mh,mw) or (B,mh,mw), float32 or uint8, of images first_index ..
        first_index+B-1.  ``disp_min`` / ``disp_max``: opt.min_depth / opt.max_depth, which upstream gives to disp_to_depth for
        both networks.  Enqueued on the current stream; nothing is synchronised.  ``export``: return the batch's per-point
        buffers {"pred": the clamped prediction before scaling, "region": the object bytes, "scaled": the prediction after
        scaling and the second clamp} (slots of the batch's segments in order; dense slots outside the mask hold NaN bits /
        0 / 0)."""
        out = self._slot(which)
        disp = self._disp_planes(disp)
        if not isinstance(doj_mask, torch.Tensor) or doj_mask.device != disp.device:
            raise _lib.MalError("accumulate: doj_mask must be a tensor on disp's device")
        if doj_mask.dtype not in (torch.float32, torch.uint8):
            raise TypeError("accumulate: doj_mask must be float32 or uint8, got %s" % doj_mask.dtype)
        doj_mask = _planes(doj_mask, "doj_mask")
        B, H, W = disp.shape
        if doj_mask.shape[0] != B:
            raise ValueError("accumulate: %d disparities, %d masks" % (B, doj_mask.shape[0]))
        first, slots = self._batch(first_index, B)
        pred = torch.empty(slots, dtype=torch.float32, device=self.device)
        region = torch.empty(slots, dtype=torch.uint8, device=self.device)
        scaled = torch.empty(slots, dtype=torch.float32, device=self.device) if export else None
        a = _lib.EvalDynArgs(n_images=self.n_images, first=first, B=B, H=H, W=W, mh=doj_mask.shape[1], mw=doj_mask.shape[2],
                             mask_dtype=_lib.EVAL_MASK_U8 if doj_mask.dtype == torch.uint8 else _lib.EVAL_MASK_F32,
                             gt_f64=int(self.gt_f64), min_depth=float(disp_min), max_depth=float(disp_max),
                             seg=self.seg.data_ptr(), idx=self.idx.data_ptr(), gt=self.gt.data_ptr(), disp=disp.data_ptr(),
                             mask=doj_mask.data_ptr(), pred=pred.data_ptr(), region=region.data_ptr(),
                             scaled=scaled.data_ptr() if export else None, img_out=out.data_ptr(),
                             stream=torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.load().mal_eval_dyn_accumulate(C.byref(a)), "mal_eval_dyn_accumulate")
        self._fed[which][first:first + B] = True
        return {"pred": pred, "region": region, "scaled": scaled} if export else None

    def rows(self, which="student"):
        """the device's (N, 18) float64 rows (include/mal_hip.h: 7 + 7 metrics, ratio, n_all, n_doj, the prediction's median)"""
        if which not in self._out:
            raise RuntimeError("rows(%r): nothing accumulated" % which)
        return self._out[which]

    def result(self, which="student"):
        """-> a dict with upstream's keys as Trainer.val leaves them in ``losses``: ``abs_rel`` .. ``a3`` (means over all
        images), ``doj/abs_rel`` .. ``doj/a3`` (sums over the images with at least one object pixel inside the mask, divided
        by their number), ``doj/count``, ``dojpxs``, ``allpxs``; and per image ``per_image`` (N,7), ``doj/per_image`` (N,7;
        zeros where ``n_doj`` is 0), ``ratios``, ``medians``, ``n_all``, ``n_doj``.  A split with ``doj/count == 0`` yields NaN
        object means, as upstream's 0/0 does.  The sums run in image order in float64 (upstream's accumulator takes a1..a3 in
        float32 or float64 depending on numpy's promotion rules).  Synchronises."""
        out = self.rows(which)
        self._all_fed(which)
        mean = torch.empty(_lib.EVAL_DYN_MEAN, dtype=torch.float64, device=self.device)
        _lib.check(_lib.load().mal_eval_dyn_mean(out.data_ptr(), self.n_images, mean.data_ptr(),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)), "mal_eval_dyn_mean")
        host, m = out.cpu().numpy(), mean.cpu().numpy()
        res = {k: m[i] for i, k in enumerate(METRICS)}
        res.update({"doj/" + k: m[7 + i] for i, k in enumerate(METRICS)})
        res.update({"doj/count": float(m[14]), "dojpxs": int(m[15]), "allpxs": int(m[16]),
                    "per_image": host[:, :7].copy(), "doj/per_image": host[:, 7:14].copy(), "ratios": host[:, 14].copy(),
                    "n_all": host[:, 15].astype(np.int64), "n_doj": host[:, 16].astype(np.int64), "medians": host[:, 17].copy()})
        return res


class DynamicDepthValPath:
    """``compute_depth_losses`` with upstream's signature, as a mixin in the manner of ``dyn_loss.DynamicDepthLossPath``.  Needs
    ``self.opt`` (min_depth, max_depth), ``self.depth_metric_names`` (upstream's seven dictionary keys in the order abs_rel,
    sq_rel, rmse, rmse_log, a1, a2, a3: "de/abs_rel" .. "da/a3", trainer.py:253-254) and ``self.dyn_evaluator``, a
    ``DynamicDepthEvaluator`` over the validation split."""

    def compute_depth_losses(self, inputs, outputs, losses, losses_mono, idx, mono, accumulate=False):
        """dynamicdepth/trainer.py:1158-1257.  ``idx``: the index of the batch's first image in the split (upstream: of its
        only image; here any batch size).  Fills the caller's dictionaries under upstream's keys -- ``metric`` and
        ``'doj/' + metric`` for ``metric in self.depth_metric_names``, ``doj/count``, ``dojpxs``, ``allpxs`` -- as upstream
        does, image by image in order: the three counts are added to ``losses`` (they must exist, as for upstream); with
        ``accumulate`` the metrics are added to (``doj/`` metrics only for images with an object pixel); without, the metrics
        of the one image are set (upstream's lines :1255-1256 have no meaning for several images: a batch raises).  Reads
        the rows back, so it synchronises, as upstream does for every metric.  ``inputs['doj_mask']`` is NOT overwritten:
        upstream's replacement by its resized first plane (:1226-1229) is a side effect nothing reads."""
        ev, opt, names = self.dyn_evaluator, self.opt, list(self.depth_metric_names)
        if len(names) != len(METRICS):
            raise ValueError("compute_depth_losses: depth_metric_names must name the %d metrics, got %r" % (len(METRICS), names))
        whos = [("student", ("disp", 0), losses)] + ([("mono", ("mono_disp", 0), losses_mono)] if mono else [])
        B = outputs[("disp", 0)].shape[0]
        if not accumulate and B != 1:
            raise ValueError("compute_depth_losses: accumulate=False sets the metrics of ONE image (trainer.py:1255-1256); "
                             "got a batch of %d" % B)
        for which, key, _ in whos:
            ev.accumulate(outputs[key], inputs["doj_mask"], idx, which, opt.min_depth, opt.max_depth)
        for which, _, dst in whos:
            rows = ev.rows(which)[idx:idx + B].cpu().numpy()
            for r in rows:
                if which == "student":   # upstream counts in ``losses`` alone, whatever ``accumulate`` is (:1231-1232, :1241)
                    dst["dojpxs"] += int(r[16])
                    dst["allpxs"] += int(r[15])
                    if r[16] > 0:
                        dst["doj/count"] += 1
                for i, metric in enumerate(names):
                    if not accumulate:
                        dst[metric] = r[i]
                        continue
                    dst[metric] += r[i]
                    if r[16] > 0:
                        dst["doj/" + metric] += r[7 + i]
