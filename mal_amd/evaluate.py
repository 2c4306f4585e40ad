"""Validation metrics on the device: upstream's ``Trainer.val`` per-image rule (manydepth/trainer.py:952-1064) and
``compute_errors`` (manydepth/evaluate_depth.py:35-53) in libmal_hip.so (csrc/mal_eval.hip).

``DepthEvaluator`` packs a split's ground truth once (valid points only: the depth mask and the split's crop depend on the
ground truth alone), then takes the network's disparities batch by batch on the caller's stream with no host
synchronisation, and ``result()`` returns what ``Trainer.val`` returns, plus the per-image errors and median ratios.
Every decision is taken in numpy's dtype (NEP 50 promotion; DESIGN.md "Validation"); the results are deterministic
and do not depend on the order or grouping of the batches.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib

__all__ = ["compute_errors", "DepthEvaluator", "pack_ground_truth", "CITYSCAPES_WINDOW", "EIGEN_CROP"]

EIGEN_CROP = (0.40810811, 0.99189189, 0.03594771, 0.96405229)   # trainer.py:1014-1015
CITYSCAPES_WINDOW = (256, 192, 1856)  # gt[256:, 192:1856] after keeping the top round(0.75 H) rows (trainer.py:985-1008)
METRICS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _device_array(t, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise _lib.MalError("%s: expected a device tensor (there is no CPU path)" % what)
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError("%s: float32 or float64, got %s" % (what, t.dtype))
    return t.contiguous().reshape(-1)


def _errors_f64(gt, pred):
    """-> (7 float64 values on the device, whether the arithmetic is float32)"""
    g, p = _device_array(gt, "gt"), _device_array(pred, "pred")
    if g.numel() != p.numel() or g.numel() == 0:
        raise ValueError("gt and pred need the same, non-zero number of elements (%d, %d)" % (g.numel(), p.numel()))
    lib = _lib.load()
    n = g.numel()
    ws = torch.empty(lib.mal_eval_errors_workspace_bytes(n), dtype=torch.uint8, device=g.device)
    out = torch.empty(7, dtype=torch.float64, device=g.device)
    _lib.check(lib.mal_eval_errors(g.data_ptr(), int(g.dtype == torch.float64), p.data_ptr(), int(p.dtype == torch.float64),
                                   n, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "mal_eval_errors")
    return out, g.dtype == torch.float32 and p.dtype == torch.float32


def compute_errors(gt, pred):
    """evaluate_depth.py:35-53 on device tensors -> (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3), 0-dim tensors in
    numpy's result dtypes: float64, except the first four when both inputs are float32 (then float32)."""
    out, f32 = _errors_f64(gt, pred)
    return tuple(out[k].float() if (f32 and k < 4) else out[k] for k in range(7))


class PackedGroundTruth(NamedTuple):
    """A split's ground truth as the kernels read it: per image one ``EvalSeg`` (include/mal_hip.h: mal_eval_seg), the valid
    points' values (a dense window's slots outside the mask hold 0) and, for the sparse splits, their flat indices."""
    segs: C.Array           # (_lib.EvalSeg * n_images)
    values: np.ndarray      # float64 or float32, the segments' slots in order
    indices: np.ndarray     # int32 flat indices into the full image, per sparse slot (one 0 if every segment is dense)
    offsets: np.ndarray     # int64 (n_images + 1,): the first slot of each image
    counts: np.ndarray      # int64 (n_images,): valid points per image
    gt_f64: bool


def pack_ground_truth(gt_depths, eval_split, min_depth, max_depth, median="numpy"):
    """-> PackedGroundTruth.  ``eval_split``: "eigen" (depth mask and Eigen crop), "cityscapes" (top round(0.75 H) rows, then
    the [256:, 192:1856] window, depth mask) or any other name (depth mask only).  ``median``: how ``med_gt`` is taken from an
    image's valid points: "numpy" (np.median: the mean of the two middle values of an even count) or "lower" (torch.median:
    the lower middle value).  Needs no device."""
    if median not in ("numpy", "lower"):
        raise ValueError("median: 'numpy' or 'lower', got %r" % (median,))
    gts = [np.asarray(g) for g in gt_depths]
    if not gts:
        raise ValueError("DepthEvaluator: no ground-truth images")
    dtypes = {g.dtype for g in gts}
    if dtypes == {np.dtype(np.float64)}:
        gt_f64 = True
    elif dtypes == {np.dtype(np.float32)}:
        gt_f64 = False
    else:
        raise ValueError("DepthEvaluator: ground truth must be all float64 or all float32, got %s" % sorted(map(str, dtypes)))
    segs = (_lib.EvalSeg * len(gts))()
    values, indices, off = [], [], 0
    for i, gt in enumerate(gts):
        if gt.ndim != 2:
            raise ValueError("DepthEvaluator: image %d: ground truth must be 2-D, got shape %s" % (i, gt.shape))
        s = segs[i]
        gh, gw = gt.shape
        if eval_split == "cityscapes":
            gh = int(round(gh * 0.75))
            y0, x0, x1 = CITYSCAPES_WINDOW
            win = gt[:gh][y0:, x0:x1]
            if win.shape != (gh - y0, x1 - x0):
                raise ValueError("DepthEvaluator: image %d: %s is too small for the cityscapes window" % (i, gt.shape))
            mask = np.logical_and(win > min_depth, win < max_depth)
            vals = np.where(mask, win, win.dtype.type(0)).reshape(-1)
            s.dense, s.x0, s.y0, s.rw = 1, x0, y0, x1 - x0
            valid = win[mask]
        else:
            mask = np.logical_and(gt > min_depth, gt < max_depth)
            if eval_split == "eigen":
                crop = np.array([EIGEN_CROP[0] * gh, EIGEN_CROP[1] * gh, EIGEN_CROP[2] * gw,
                                 EIGEN_CROP[3] * gw]).astype(np.int32)
                crop_mask = np.zeros(mask.shape)
                crop_mask[crop[0]:crop[1], crop[2]:crop[3]] = 1
                mask = np.logical_and(mask, crop_mask)
            ys, xs = np.nonzero(mask)
            indices.append((ys * gw + xs).astype(np.int32))
            vals = valid = gt[mask]
        if valid.size == 0:
            raise ValueError("DepthEvaluator: image %d has no valid ground-truth pixel (%s < gt < %s%s); upstream's "
                             "metrics would be NaN" % (i, min_depth, max_depth, " inside the crop" if eval_split in
                                                       ("eigen", "cityscapes") else ""))
        s.off, s.slots, s.n, s.gt_h, s.gt_w = off, vals.size, valid.size, gh, gw
        if median == "numpy":
            s.med_gt = float(np.median(valid))  # exact in its dtype
        else:
            k = (valid.size - 1) // 2
            s.med_gt = float(np.partition(valid, k)[k])
        values.append(vals)
        off += vals.size
    return PackedGroundTruth(segs, np.concatenate(values), np.concatenate(indices) if indices else np.zeros(1, np.int32),
                             np.array([s.off for s in segs] + [off], np.int64), np.array([s.n for s in segs], np.int64), gt_f64)


def _planes(t, what):
    """(B,1,h,w) | (B,h,w) -> contiguous (B,h,w)"""
    if t.dim() == 4:
        if t.shape[1] != 1:
            raise ValueError("accumulate: %s must be (B,1,h,w), got %s" % (what, tuple(t.shape)))
        t = t[:, 0]
    if t.dim() != 3:
        raise ValueError("accumulate: %s must be (B,1,h,w) or (B,h,w), got %s" % (what, tuple(t.shape)))
    return t.contiguous()


class _SplitEvaluator:
    """What DepthEvaluator and dyn_eval.DynamicDepthEvaluator do alike: a split's packed ground truth on the device, one
    (n_images, ROW) float64 row tensor per network ("student", "mono"), and the book-keeping of which images were fed."""
    ROW = 8

    def _upload(self, pk):
        self.n_images, self.gt_f64, self.offsets, self.counts = len(pk.segs), pk.gt_f64, pk.offsets, pk.counts
        self.gt = torch.from_numpy(pk.values).to(self.device)
        self.idx = torch.from_numpy(pk.indices).to(self.device)
        self.seg = torch.frombuffer(bytearray(bytes(pk.segs)), dtype=torch.uint8).to(self.device)
        self.reset()

    def reset(self):
        self._out, self._fed = {}, {}

    def _slot(self, which):
        if which not in ("student", "mono"):
            raise ValueError("which: 'student' or 'mono', got %r" % (which,))
        if which not in self._out:
            self._out[which] = torch.zeros(self.n_images, self.ROW, dtype=torch.float64, device=self.device)
            self._fed[which] = np.zeros(self.n_images, bool)
        return self._out[which]

    @staticmethod
    def _disp_planes(disp):
        if not isinstance(disp, torch.Tensor) or disp.device.type != "cuda" or disp.dtype != torch.float32:
            raise _lib.MalError("accumulate: disp must be a float32 device tensor (there is no CPU path)")
        return _planes(disp, "disp")

    def _batch(self, first_index, B):
        """-> (index of the batch's first image, number of packed slots of its B images)"""
        first = int(first_index)
        if first < 0 or first + B > self.n_images:
            raise IndexError("accumulate: images %d..%d outside the split's %d" % (first, first + B - 1, self.n_images))
        return first, int(self.offsets[first + B] - self.offsets[first])

    def _all_fed(self, which):
        missing = np.nonzero(~self._fed[which])[0]
        if missing.size:
            raise RuntimeError("result(%r): %d image(s) never accumulated, first %d" % (which, missing.size, missing[0]))


class DepthEvaluator(_SplitEvaluator):
    """The per-image half of ``Trainer.val`` (trainer.py:952-1064) for one split.

    ``gt_depths``: the split's ground truth, a list of 2-D numpy arrays of ragged sizes, all float64 (KITTI's
    gt_depths.npz) or all float32.  ``eval_split``: "eigen" (depth mask and Eigen crop), "cityscapes" (top round(0.75 H)
    rows, then the [256:, 192:1856] window, depth mask) or any other name (depth mask only).  Upstream returns NaN
    metrics for an image with no valid pixel (the median of an empty slice); here such an image raises ValueError, naming
    it, at construction.
    """

    def __init__(self, gt_depths, eval_split, device="cuda", min_depth=1e-3, max_depth=80):
        self.split, self.device = eval_split, torch.device(device)
        self.min_depth, self.max_depth = min_depth, max_depth
        self._upload(pack_ground_truth(gt_depths, eval_split, min_depth, max_depth, "numpy"))

    def reset(self):
        super().reset()
        self._scaled = {}

    def accumulate(self, disp, first_index, which="student", disp_min=1e-3, disp_max=80, median_scaling=True,
                   scale_factor=1.0, _resize_ulp=0):
        """One batch: ``disp`` (B,1,h,w) or (B,h,w) float32 sigmoid outputs of images first_index .. first_index+B-1.
        ``disp_min`` / ``disp_max``: the min_depth / max_depth given to disp_to_depth (the student: 1e-3, 80,
        trainer.py:952; the teacher: 1e-3, opt.max_depth, :959).  ``median_scaling``: not opt.disable_median_scaling
        for the student, always True for the teacher (which="mono"); ``scale_factor``: opt.pred_depth_scale_factor for
        the student, 1 for the teacher.  Enqueued on the current stream; nothing is synchronised."""
        out = self._slot(which)
        disp = self._disp_planes(disp)
        B, H, W = disp.shape
        first, slots = self._batch(first_index, B)
        if self._scaled.setdefault(which, bool(median_scaling)) != bool(median_scaling):
            raise ValueError("accumulate: median_scaling changed between batches of %r" % which)
        lib = _lib.load()
        pred = torch.empty(slots, dtype=torch.float32, device=self.device)
        a = _lib.EvalArgs(n_images=self.n_images, first=first, B=B, H=H, W=W, gt_f64=int(self.gt_f64),
                          median_scaling=int(bool(median_scaling)), resize_ulp=int(_resize_ulp),
                          min_depth_disp=float(disp_min), max_depth_disp=float(disp_max), scale_factor=float(scale_factor),
                          clamp_min=float(self.min_depth), clamp_max=float(self.max_depth),
                          seg=self.seg.data_ptr(), idx=self.idx.data_ptr(), gt=self.gt.data_ptr(), disp=disp.data_ptr(),
                          pred=pred.data_ptr(), img_out=out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.mal_eval_accumulate(C.byref(a)), "mal_eval_accumulate")
        self._fed[which][first:first + B] = True

    def result(self, which="student"):
        """-> (mean_errors (7,), per-image errors (N, 7), ratios (N,) or None without median scaling), float64 numpy:
        abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 as Trainer.val's ``np.array(errors).mean(0)``.  Synchronises."""
        if which not in self._out:
            raise RuntimeError("result(%r): nothing accumulated" % which)
        self._all_fed(which)
        lib = _lib.load()
        out = self._out[which]
        mean = torch.empty(7, dtype=torch.float64, device=self.device)
        _lib.check(lib.mal_eval_mean(out.data_ptr(), self.n_images, mean.data_ptr(), _stream()), "mal_eval_mean")
        host = out.cpu().numpy()
        ratios = host[:, 7].copy() if self._scaled[which] else None
        if ratios is not None and not self.gt_f64:
            ratios = ratios.astype(np.float32)
        return mean.cpu().numpy(), host[:, :7].copy(), ratios
