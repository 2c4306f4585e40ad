"""CPU oracle (numpy) of upstream's validation metrics: Trainer.val's per-image rule (manydepth/trainer.py:836-1064) and
compute_errors (manydepth/evaluate_depth.py:35-53), with a restatement of cv2.resize(INTER_LINEAR) on float32 images.

cv2.resize, restated from a reading of OpenCV's generic path (imgproc/src/resize.cpp: resize -> resizeGeneric_ with
HResizeLinear<float, float, float, 1, HResizeNoVec> and VResizeLinear<float, float, float, Cast, VResizeLinearVec_32f>):
  * scale = 1 / (double(dst) / src); per destination column f = float((d + 0.5) * scale - 0.5), s = floor(f), f -= s,
    both in float; the same per destination row.
  * columns: s < 0 -> (s, f) = (0, 0); s >= src - 1 -> (s, f) = (src - 1, 0) and the column is a plain copy of the edge
    pixel (HResizeLinear's dx >= xmax tail); otherwise S[s] * (1 - f) + S[s + 1] * f in float.
  * rows: both taps clamped into the image, the fractional weight kept: H[clamp(s)] * (1 - f) + H[clamp(s + 1)] * f.
What could not be confirmed here (no OpenCV source or binary on the authoring machine):
  * whether a given build routes float INTER_LINEAR through IPP or a HAL (cv_hal_resize) instead of resizeGeneric_;
  * whether the vertical pass is fused: VResizeLinearVec_32f computes v_muladd(S0, b0, S1 * b1), which is one FMA when
    the build enables FMA3 / NEON-FMA dispatch and a multiply plus an add otherwise.  ``fma_vertical=True`` gives the
    fused form; the product (and the default here) is unfused.  test_gpu_eval.py measures how far the metrics move when
    every resized value moves by one ulp, which bounds either difference.
Disparities are float32, so every product and sum above is a float32 operation with one rounding.
"""
from __future__ import annotations

import numpy as np

MIN_VAL, MAX_VAL = 1e-3, 80          # trainer.py:841-842
EIGEN_CROP = (0.40810811, 0.99189189, 0.03594771, 0.96405229)   # trainer.py:1014-1015
CITYSCAPES_WINDOW = (256, 192, 1856)  # gt[256:, 192:1856] after keeping the top round(0.75 H) rows (trainer.py:985-1008)
KITTI_GT_SIZES = [(375, 1242), (370, 1224), (374, 1238), (370, 1226), (376, 1241)]  # the raw recording days' image sizes


def disp_to_depth(disp, min_depth, max_depth):
    """manydepth/layers.py:14-23 on float32 arrays (torch's scalar arithmetic: both constants rounded to float32)"""
    min_disp = 1 / max_depth
    max_disp = 1 / min_depth
    scaled = np.float32(min_disp) + np.float32(max_disp - min_disp) * np.asarray(disp, np.float32)
    return scaled, np.float32(1) / scaled


def _taps(n_dst, n_src):
    scale = 1.0 / (float(n_dst) / n_src)
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    return s, f


def _columns(sw, dw):
    sx, fx = _taps(dw, sw)
    fx = fx.copy()
    left = sx < 0
    sx[left], fx[left] = 0, 0
    copy = sx >= sw - 1
    sx[copy], fx[copy] = sw - 1, 0
    return sx, fx, copy


def _rows(sh, dh):
    sy, fy = _taps(dh, sh)
    return np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1), fy


def _vertical(h0, h1, b0, b1, fma_vertical):
    if fma_vertical:  # fma(h0, b0, h1 * b1), exact in float64 before the single rounding to float32
        return (h0.astype(np.float64) * b0 + (h1 * b1).astype(np.float64)).astype(np.float32)
    return h0 * b0 + h1 * b1


def resize_linear(src, dst_w, dst_h, fma_vertical=False):
    """cv2.resize(src, (dst_w, dst_h)) for a 2-D float32 image, INTER_LINEAR, as the two passes OpenCV runs"""
    src = np.asarray(src, np.float32)
    sh, sw = src.shape
    sx, fx, copy = _columns(sw, dst_w)
    a0, a1 = np.float32(1) - fx, fx
    sx1 = np.minimum(sx + 1, sw - 1)
    H = src[:, sx] * a0 + src[:, sx1] * a1
    H[:, copy] = src[:, sx[copy]]
    y0, y1, fy = _rows(sh, dst_h)
    b0, b1 = (np.float32(1) - fy)[:, None], fy[:, None]
    return _vertical(H[y0], H[y1], b0, b1, fma_vertical)


def resize_at(src, dst_w, dst_h, ys, xs, fma_vertical=False):
    """resize_linear(src, dst_w, dst_h)[ys, xs] evaluated only at those pixels, in the same operation order"""
    src = np.asarray(src, np.float32)
    sh, sw = src.shape
    sx, fx, copy = _columns(sw, dst_w)
    y0, y1, fy = _rows(sh, dst_h)
    cx, c0, cc = sx[xs], fx[xs], copy[xs]
    c1 = np.minimum(cx + 1, sw - 1)
    a0, a1 = np.float32(1) - c0, c0

    def h(r):
        v = src[r, cx] * a0 + src[r, c1] * a1
        return np.where(cc, src[r, cx], v)
    r0, r1, f = y0[ys], y1[ys], fy[ys]
    return _vertical(h(r0), h(r1), np.float32(1) - f, f, fma_vertical)


def eigen_crop(h, w):
    """trainer.py:1014-1016: the float64 products truncated by astype(np.int32) -> (top, bottom, left, right)"""
    return np.array([EIGEN_CROP[0] * h, EIGEN_CROP[1] * h, EIGEN_CROP[2] * w, EIGEN_CROP[3] * w]).astype(np.int32)


def _log(x, cr_log):
    """np.log; with cr_log the log of a float32 array is the correctly rounded float32(log(float64(x))), which is what the
    device computes (logf_cr), where numpy's SIMD logf is a few ulp off"""
    if cr_log and np.asarray(x).dtype == np.float32:
        return np.log(np.asarray(x).astype(np.float64)).astype(np.float32)
    return np.log(x)


def compute_errors(gt, pred, cr_log=False):
    """evaluate_depth.py:35-53 (numpy promotion decides every dtype).  cr_log: see _log; it moves rmse_log only."""
    thresh = np.maximum((gt / pred), (pred / gt))
    a1 = (thresh < 1.25).mean()
    a2 = (thresh < 1.25 ** 2).mean()
    a3 = (thresh < 1.25 ** 3).mean()
    rmse = (gt - pred) ** 2
    rmse = np.sqrt(rmse.mean())
    rmse_log = (_log(gt, cr_log) - _log(pred, cr_log)) ** 2
    rmse_log = np.sqrt(rmse_log.mean())
    abs_rel = np.mean(np.abs(gt - pred) / gt)
    sq_rel = np.mean(((gt - pred) ** 2) / gt)
    return abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3


def valid_points(gt_depth, split, min_depth=MIN_VAL, max_depth=MAX_VAL):
    """-> (gt cropped to what the prediction is resized to, its (h, w), (ys, xs) of the valid points, window origin)
    (trainer.py:983-1020): the cityscapes top crop and window, the depth mask, the eigen crop"""
    gt_depth = np.asarray(gt_depth)
    gh, gw = gt_depth.shape[:2]
    y0 = x0 = 0
    if split == "cityscapes":
        gh = int(round(gh * 0.75))
        gt_depth = gt_depth[:gh]
        y0, x0, x1 = CITYSCAPES_WINDOW
        win = gt_depth[y0:, x0:x1]
    else:
        win = gt_depth
    mask = np.logical_and(win > min_depth, win < max_depth)
    if split == "eigen":
        crop = eigen_crop(gh, gw)
        crop_mask = np.zeros(mask.shape)
        crop_mask[crop[0]:crop[1], crop[2]:crop[3]] = 1
        mask = np.logical_and(mask, crop_mask)
    ys, xs = np.nonzero(mask)
    return win, (gh, gw), (ys + y0, xs + x0), mask


def evaluate_image(gt_depth, pred_disp, split, median_scaling=True, scale_factor=None, min_depth=MIN_VAL,
                   max_depth=MAX_VAL, fma_vertical=False, ulp=0, pointwise=True, cr_log=False):
    """one image of Trainer.val (trainer.py:998-1051) for a float32 scaled disparity (h, w).  scale_factor None: the
    teacher's rule (no pred_depth_scale_factor).  ulp: move every resized disparity by that many ulps.  pointwise: resize
    only at the valid points (same values as the full two-pass image, test_eval_oracle.py holds that).  cr_log: as in
    compute_errors.
    -> dict(errors, ratio (None without median scaling), pred (clamped, float32), gt (masked), n)"""
    win, (gh, gw), (ys, xs), mask = valid_points(gt_depth, split, min_depth, max_depth)
    if pointwise:
        pd = resize_at(pred_disp, gw, gh, ys, xs, fma_vertical)
    else:
        full = resize_linear(pred_disp, gw, gh, fma_vertical)
        pd = full[ys, xs]
    if ulp:
        pd = (pd.view(np.uint32) + np.uint32(ulp) if ulp > 0 else pd.view(np.uint32) - np.uint32(-ulp)).view(np.float32)
    pred = np.float32(1) / pd
    gt = win[mask]
    if scale_factor is not None:
        pred *= scale_factor
    ratio = None
    if median_scaling:
        ratio = np.median(gt) / np.median(pred)
        pred *= ratio
    pred[pred < min_depth] = min_depth
    pred[pred > max_depth] = max_depth
    return dict(errors=compute_errors(gt, pred, cr_log), ratio=ratio, pred=pred, gt=gt, n=int(gt.size))


def evaluate(gt_depths, disps, split, median_scaling=True, scale_factor=None, **kw):
    """-> (mean_errors, per-image errors (N, 7), ratios) for scaled disparities (N, h, w)"""
    rows, ratios = [], []
    for i in range(len(disps)):
        r = evaluate_image(gt_depths[i], disps[i], split, median_scaling, scale_factor, **kw)
        rows.append(r["errors"])
        if r["ratio"] is not None:
            ratios.append(r["ratio"])
    errs = np.array(rows)
    return errs.mean(0), errs, np.array(ratios)


# ---------------------------------------------------------------- synthetic sets (seeded; plain IEEE arithmetic only, so
# every machine generates the same bits)
def _smooth(rng, h, w, gh, gw):
    """a (h, w) float64 field in [0, 1): bilinear upsampling of a (gh, gw) random grid"""
    g = rng.random((gh, gw))
    y = np.arange(h) * ((gh - 1) / max(h - 1, 1))
    x = np.arange(w) * ((gw - 1) / max(w - 1, 1))
    y0 = np.minimum(y.astype(np.int64), gh - 2)
    x0 = np.minimum(x.astype(np.int64), gw - 2)
    fy, fx = (y - y0)[:, None], (x - x0)[None, :]
    top = g[y0][:, x0] * (1 - fx) + g[y0][:, x0 + 1] * fx
    bot = g[y0 + 1][:, x0] * (1 - fx) + g[y0 + 1][:, x0 + 1] * fx
    return top * (1 - fy) + bot * fy


def disparities(seed, n, h, w, flat=0.3, extremes=True):
    """network-like sigmoid outputs (n, 1, h, w) float32 (depths of ~0.2 to 10 through disp_to_depth(., 1e-3, 80)):
    smooth fields, a share of pixels quantised to 2^-13 (exact ties), and some at 1e-6 and 1 (depths that end up clamped)"""
    rng = np.random.default_rng(seed)
    out = np.empty((n, 1, h, w), np.float32)
    for i in range(n):
        d = 1e-4 + 0.004 * _smooth(rng, h, w, 5, 9) + 0.001 * rng.random((h, w))
        q = rng.random((h, w)) < flat
        d[q] = np.round(d[q] * 8192) / 8192
        if extremes:
            e = rng.random((h, w))
            d[e < 0.01] = 1e-6
            d[e > 0.995] = 1.0
        out[i, 0] = d
    return out


def kitti_gt(seed, n, sizes=KITTI_GT_SIZES, density=0.04, dtype=np.float64):
    """LiDAR-like sparse ground truth (synthetic): ~density of the pixels below the top 25 % hold a depth, a few outside
    the (1e-3, 80) mask; ragged sizes cycling through ``sizes``"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        gt = np.zeros((h, w), np.float64)
        field = 2.0 + 60.0 * _smooth(rng, h, w, 4, 8)
        pick = rng.random((h, w)) < density
        pick[: h // 4] = False
        vals = field * (0.9 + 0.2 * rng.random((h, w)))
        far = rng.random((h, w)) < 0.01
        vals[far] = 85.0
        tie = rng.random((h, w)) < 0.2
        vals[tie] = np.round(vals[tie] * 4) / 4
        gt[pick] = vals[pick]
        out.append(gt.astype(dtype))
    return out


def cityscapes_gt(seed, n, h=1024, w=2048, dtype=np.float32):
    """dense CityScapes-like ground truth (synthetic): 0 where there is no depth, a few values past 80"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        d = 3.0 + 70.0 * _smooth(rng, h, w, 6, 10) + 15.0 * rng.random((h, w))
        d[rng.random((h, w)) < 0.1] = 0.0
        out.append(d.astype(dtype))
    return out


def kitti_sparse_gt(seed, n, sizes=KITTI_GT_SIZES, density=0.04, dtype=np.float64):
    """a cheaper LiDAR-like set for many full-size images (synthetic): ~density*h*w points drawn uniformly below the top
    quarter (a repeated position keeps the last draw), depths 2..70 with a share rounded to 1/4 m (ties) and 1 % at 85"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        m = int(density * h * w)
        ys = rng.integers(h // 4, h, m)
        xs = rng.integers(0, w, m)
        v = 2.0 + 68.0 * rng.random(m)
        t = rng.random(m)
        v[t < 0.2] = np.round(v[t < 0.2] * 4) / 4
        v[t > 0.99] = 85.0
        gt = np.zeros((h, w), np.float64)
        gt[ys, xs] = v
        out.append(gt.astype(dtype))
    return out
