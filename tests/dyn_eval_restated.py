"""DynamicDepth's validation rule restated in plain torch: ``Trainer.compute_depth_losses`` (dynamicdepth/trainer.py:1158-1257),
``layers.compute_depth_errors`` (dynamicdepth/layers.py:244-262) and the aggregation at the end of ``Trainer.val`` (:881-905).

TEST INFRASTRUCTURE ONLY: what csrc/mal_dyn_eval.hip is held to.  Two dtypes:

  torch.float32  upstream's arithmetic operation for operation -- equal to the reference's fixtures (tests/golden/dyn_eval_*.npz,
                 scripts/gen_golden_dyn_eval.py) BIT FOR BIT on the CPU (tests/test_dyn_eval_cases.py)
  torch.float64  the same function with the prediction carried in float64: what a float32 evaluation is measured against

The bilinear taps (ATen's upsample_bilinear2d, align_corners=False) and the nearest rule (upsample_nearest2d) are written
out (``resize_bilinear``, ``resize_nearest``), which is what lets the float64 form and the one-edit variants exist.  The
float32 form on the CPU calls ``F.interpolate`` for the bilinear resize all the same (``resize="aten"``): ATen's CPU build
contracts ``scale * (dst + 0.5) - 0.5`` and the weighted sums into fused multiply-adds, so no sequence of separately rounded
torch operators gives its bits; the written-out float32 form stays within a few ulp of a tap difference of it
(tests/test_dyn_eval_cases.py measures the distance), and the nearest rule is exact.  ``forced``: the
device's own decisions replace the restatement's -- ``median_index`` (the position, among the valid points, of the value taken
as the prediction's median) and ``lt`` (the three ``thresh < 1.25 ** k`` comparisons).

The case tables at the bottom are seeded numpy; every seed was picked so that the case is ADMISSIBLE in this file's float32
arithmetic alone (no ``thresh`` within 1e-4 relative of a threshold), which tests/test_dyn_eval_cases.py asserts.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

METRICS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")
EIGEN_CROP = (0.40810811, 0.99189189, 0.03594771, 0.96405229)   # trainer.py:1207-1208
CITYSCAPES_WINDOW = (256, 192, 1856)                            # trainer.py:1199
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)
CLAMP = (1e-3, 80)                                              # trainer.py:1189, :1220: literals
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------- pieces
def disp_to_depth(disp, min_depth, max_depth):
    """layers.py:8-17, the depth; the Python floats meet the tensor as torch's scalars do"""
    min_disp = 1 / max_depth
    max_disp = 1 / min_depth
    return 1 / (min_disp + (max_disp - min_disp) * disp)


def bilinear_taps(n_dst, n_src, dtype, lam_before_max=False):
    """ATen's area_pixel_compute_source_index + upsample_bilinear2d's taps -> (i0, i1, l0, l1).  The scale is
    (accscalar)in / out: float32 for a float32 input, float64 for a float64 one."""
    dst = torch.arange(n_dst, dtype=dtype)
    scale = torch.tensor(n_src, dtype=dtype) / torch.tensor(n_dst, dtype=dtype)
    raw = scale * (dst + 0.5) - 0.5
    src = torch.clamp(raw, min=0)
    i0 = src.to(torch.int64)
    i1 = i0 + (i0 < n_src - 1).to(torch.int64)
    l1 = (raw if lam_before_max else src) - i0.to(dtype)
    return i0, i1, 1 - l1, l1


def resize_bilinear(depth, gh, gw, **kw):
    """F.interpolate(depth (h,w), [gh,gw], mode="bilinear", align_corners=False) in the device kernel's operation order"""
    y0, y1, l0y, l1y = bilinear_taps(gh, depth.shape[0], depth.dtype, **kw)
    x0, x1, l0x, l1x = bilinear_taps(gw, depth.shape[1], depth.dtype, **kw)
    top = l0x * depth[y0][:, x0] + l1x * depth[y0][:, x1]
    bot = l0x * depth[y1][:, x0] + l1x * depth[y1][:, x1]
    return l0y[:, None] * top + l1y[:, None] * bot


def nearest_index(n_dst, n_src, half=False):
    """ATen's nearest_neighbor_compute_source_index: min(floor(dst * (float)in / out), in - 1), in float32 whatever the data"""
    scale = torch.tensor(n_src, dtype=torch.float32) / torch.tensor(n_dst, dtype=torch.float32)
    dst = torch.arange(n_dst, dtype=torch.float32) + (0.5 if half else 0.0)
    return torch.clamp(torch.floor(dst * scale).to(torch.int64), max=n_src - 1)


def resize_nearest(m, gh, gw, **kw):
    return m[nearest_index(gh, m.shape[0], **kw)][:, nearest_index(gw, m.shape[1], **kw)]


def lower_median(v):
    """torch.median of a 1-D tensor: element (n - 1) // 2 of the sorted values -> (0-dim value, index into v)"""
    order = torch.argsort(v, stable=True)
    i = order[(v.numel() - 1) // 2]
    return v[i], int(i)


def eigen_crop(gh, gw):
    c = np.array([EIGEN_CROP[0] * gh, EIGEN_CROP[1] * gh, EIGEN_CROP[2] * gw, EIGEN_CROP[3] * gw]).astype(np.int32)
    return int(c[0]), int(c[1]), int(c[2]), int(c[3])


def valid_points(gt_depth, split):
    """-> (gt cropped as upstream crops it, mask over it, (gh, gw) the prediction is resized to, (y0, x0) of the cropped
    array inside that size)"""
    gt = np.asarray(gt_depth)
    gh, gw = gt.shape
    if split == "cityscapes":
        gh = int(round(gh * 0.75))
        y0, x0, x1 = CITYSCAPES_WINDOW
        gt = gt[:gh][y0:, x0:x1]
        return gt, np.logical_and(gt > CLAMP[0], gt < CLAMP[1]), (gh, gw), (y0, x0)
    if split not in ("eigen", "eigen_benchmark"):
        raise ValueError("upstream leaves `mask` undefined for eval_split %r" % (split,))
    mask = np.logical_and(gt > CLAMP[0], gt < CLAMP[1])
    c = eigen_crop(gh, gw)
    crop_mask = np.zeros(mask.shape)
    crop_mask[c[0]:c[1], c[2]:c[3]] = 1
    return gt, np.logical_and(mask, crop_mask), (gh, gw), (0, 0)


def _log_own(x, dtype):
    """torch.log in the operand's OWN dtype, delivered in ``dtype``: in the float64 form a float32 operand's log is the
    correctly rounded float32 value (what the device takes)"""
    if dtype == torch.float64 and x.dtype == torch.float32:
        return torch.log(x.double()).float().double()
    return torch.log(x)


def compute_depth_errors(gt, pred, dtype=torch.float32, forced_lt=None):
    """layers.py:244-262 -> 7 0-dim tensors.  float32: upstream's lines on the tensors as they come (torch promotes a float32
    prediction to a float64 ground truth's dtype).  float64: everything but the logs (see _log_own) in float64."""
    lg, lp = _log_own(gt, dtype), _log_own(pred, dtype)
    if dtype == torch.float64:
        gt, pred = gt.double(), pred.double()
    thresh = torch.max((gt / pred), (pred / gt))
    lt = [thresh < t for t in THRESHOLDS] if forced_lt is None else [x.bool() for x in forced_lt]
    a1, a2, a3 = (x.float().mean() for x in lt)
    rmse = (gt - pred) ** 2
    rmse = torch.sqrt(rmse.mean())
    rmse_log = (lg - lp) ** 2
    rmse_log = torch.sqrt(rmse_log.mean())
    abs_rel = torch.mean(torch.abs(gt - pred) / gt)
    sq_rel = torch.mean((gt - pred) ** 2 / gt)
    return abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3


def thresh_margin(gt, pred):
    """the smallest relative distance of a point's ``thresh`` from a threshold"""
    thresh = torch.max((gt / pred), (pred / gt)).double()
    return min(float(((thresh - t).abs() / t).min()) for t in THRESHOLDS)


# ---------------------------------------------------------------- one image, one split
def evaluate_image(gt_depth, disp, doj_mask, split, min_depth, max_depth, dtype=torch.float32, forced=None, variant=None,
                   resize=None):
    """trainer.py:1158-1257 for one image: ``disp`` (h,w) float32, ``doj_mask`` (mh,mw) any dtype.  ``variant``: a one-edit
    departure from the rule (tests only): "upper", "mean2", "noclamp1", "nearest_half", "lam_before_max".  ``resize``: "aten"
    (F.interpolate; the default in float32) or "explicit" (resize_bilinear; the default in float64 and for the tap variant)."""
    if resize is None:
        resize = "aten" if dtype == torch.float32 and variant != "lam_before_max" else "explicit"
    gt_np, mask_np, (gh, gw), (y0, x0) = valid_points(gt_depth, split)
    d = disp.to(dtype)
    depth = disp_to_depth(d, min_depth, max_depth)
    if resize == "aten":
        full = F.interpolate(depth[None, None], [gh, gw], mode="bilinear", align_corners=False)[0, 0]
    else:
        full = resize_bilinear(depth, gh, gw, lam_before_max=variant == "lam_before_max")
    if variant != "noclamp1":
        full = torch.clamp(full, CLAMP[0], CLAMP[1])
    pred = full[y0:y0 + gt_np.shape[0], x0:x0 + gt_np.shape[1]].clone()
    gt = torch.from_numpy(np.ascontiguousarray(gt_np))
    mask = torch.from_numpy(mask_np)
    if int(mask.sum()) == 0:
        raise ValueError("no valid ground-truth pixel")
    pts = pred[mask]
    med_gt, _ = lower_median(gt[mask])
    med_pred, med_index = lower_median(pts)
    if variant in ("upper", "mean2"):
        up = torch.sort(pts)[0][pts.numel() // 2]
        med_pred = up if variant == "upper" else (med_pred + up) / 2
    if forced is not None and "median_index" in forced:
        med_index = int(forced["median_index"])
        med_pred = pts[med_index]
    ratio = med_gt / med_pred            # two 0-dim tensors: their promoted dtype
    first = pts.clone()
    pred *= ratio                        # in place: the map's dtype; the 0-dim operand is cast to it first
    pred = torch.clamp(pred, min=CLAMP[0], max=CLAMP[1])
    region = resize_nearest(doj_mask, gh, gw, half=variant == "nearest_half")
    region = region[y0:y0 + gt_np.shape[0], x0:x0 + gt_np.shape[1]]
    doj = mask * region.bool()
    out = {"pred_full": full, "pred_first": first, "pred": pred[mask], "gt": gt[mask], "mask": mask, "doj_mask": doj,
           "region": region.bool()[mask], "ratio": ratio, "median": med_pred, "median_index": med_index,
           "n_all": int(mask.sum()), "n_doj": int(doj.sum())}
    lt_all = None if forced is None else forced.get("lt")
    out["errors"] = compute_depth_errors(gt[mask], pred[mask], dtype, lt_all)
    if out["n_doj"] > 0:
        lt_doj = None if lt_all is None else [x[out["region"]] for x in lt_all]
        out["doj_errors"] = compute_depth_errors(gt[doj], pred[doj], dtype, lt_doj)
    else:
        out["doj_errors"] = None
    out["margin"] = thresh_margin(gt[mask], pred[mask])
    return out


def aggregate(images):
    """what Trainer.val leaves in ``losses`` (:760-766, :1231-1252, :881-886): sums in image order in float64"""
    losses = {m: 0.0 for m in METRICS}
    losses.update({"doj/" + m: 0.0 for m in METRICS})
    losses.update({"doj/count": 0.0, "dojpxs": 0, "allpxs": 0})
    for r in images:
        losses["dojpxs"] += r["n_doj"]
        losses["allpxs"] += r["n_all"]
        if r["n_doj"] > 0:
            losses["doj/count"] += 1
        for i, m in enumerate(METRICS):
            losses[m] += float(r["errors"][i])
            if r["n_doj"] > 0:
                losses["doj/" + m] += float(r["doj_errors"][i])
    for m in METRICS:
        losses[m] /= float(len(images))
        losses["doj/" + m] = losses["doj/" + m] / losses["doj/count"] if losses["doj/count"] else float("nan")
    return losses


def evaluate_case(c, which="student", dtype=torch.float32, forced=None, variant=None, resize=None):
    disp = c["disp"] if which == "student" else c["mono_disp"]
    return [evaluate_image(c["gt"][i], disp[i, 0], c["doj_mask"][i, 0], c["split"], c["min_depth"], c["max_depth"], dtype,
                           None if forced is None else forced[i], variant, resize) for i in range(len(c["gt"]))]


# ---------------------------------------------------------------- case tables
# name: (split, disp (h,w), gt (H,W), gt dtype, mask (h,w), mask dtype, valid counts per image, (min_depth, max_depth), seed)
# The images of a case carry, in turn, a random object mask, an empty one and a full one.
SWEEP_CASES = {
    "d1x1":      ("eigen", (1, 1), (9, 13), "f8", (1, 1), "f4", (1, 2, 3), (0.1, 100.0), 0),
    "d1x7":      ("eigen", (1, 7), (9, 13), "f4", (4, 5), "u1", (4,), (0.1, 100.0), 0),
    "d5x1":      ("eigen", (5, 1), (9, 13), "f8", (5, 1), "u1", (3, 4, 1), (0.1, 100.0), 0),
    "d2x2":      ("eigen", (2, 2), (9, 13), "f4", (9, 13), "f4", (2,), (0.1, 100.0), 0),
    "same6x10":  ("eigen", (6, 10), (6, 10), "f8", (6, 10), "f4", (4, 3, 2), (0.1, 100.0), 0),
    "ulps6x10":  ("eigen", (6, 10), (6, 10), "f4", (6, 10), "u1", (9, 8, 6), (0.1, 100.0), 0),   # odd, even, all equal (below)
    "up7x11":    ("eigen", (6, 10), (7, 11), "f4", (3, 4), "u1", (24,), (0.1, 100.0), 0),
    "up12x20":   ("eigen", (3, 5), (12, 20), "f8", (3, 5), "f4", (40, 41, 17), (0.1, 100.0), 0),
    "clamps":    ("eigen", (3, 5), (12, 20), "f4", (6, 10), "f4", (60, 61, 33), (5e-4, 100.0), 0),
    "nodoj":     ("eigen", (3, 5), (12, 20), "f4", (3, 5), "u1", (25,), (0.1, 100.0), 0),   # one image, empty mask: doj/count 0
    "eigen1024": ("eigen", (24, 64), (93, 310), "f8", (24, 64), "f4", (1023, 1024, 1025), (0.1, 100.0), 3),
    "eigen2049": ("eigen", (24, 64), (93, 310), "f4", (12, 32), "u1", (2049,), (0.1, 100.0), 11),
    "city2":     ("cityscapes", (6, 16), (344, 2048), "f4", (6, 16), "u1", (1200,), (0.1, 100.0), 0),
    "city3":     ("cityscapes", (12, 32), (345, 2048), "f8", (24, 64), "f4", (300, 500, 900), (0.1, 100.0), 1),
}
GOLDEN_CASES = {
    "eigen_24x64": ("eigen", (24, 64), (93, 310), "f8", (24, 64), "f4", (601, 600, 450), (0.1, 100.0), 0),
    "eigen_3x5":   ("eigen_benchmark", (3, 5), (12, 20), "f8", (6, 10), "f4", (36, 37, 20), (0.1, 100.0), 0),
    "cityscapes":  ("cityscapes", (12, 32), (1024, 2048), "f4", (12, 32), "f4", (300, 301), (0.1, 100.0), 1),
}


ULPS_BASE = np.float32(0.00901)   # disp_to_depth(., 0.1, 100) = 9.99901, bits 0x411ffbf2


def valid_region(split, H, W):
    """the rectangle (y0, y1, x0, x1) of the full ground truth that can hold a valid point"""
    if split == "cityscapes":
        y0, x0, x1 = CITYSCAPES_WINDOW
        return y0, int(round(H * 0.75)), x0, x1
    return eigen_crop(H, W)


def make_case(name, table=None, seed=None):
    table = table or (SWEEP_CASES if name in SWEEP_CASES else GOLDEN_CASES)
    split, (h, w), (H, W), gdt, (mh, mw), mdt, counts, (dmin, dmax), s = table[name]
    rng = np.random.default_rng([sum(name.encode()), s if seed is None else seed])
    B = len(counts)
    y0, y1, x0, x1 = valid_region(split, H, W)
    gts = []
    for i, n in enumerate(counts):
        g = np.zeros((H, W), np.dtype(gdt))
        cells = rng.choice((y1 - y0) * (x1 - x0), size=n, replace=False)
        if n >= 2:
            cells[0] = 0   # the first column (and the window's first row): where max(0, .) clamps the source coordinate
        cells = np.unique(cells)
        while cells.size < n:
            cells = np.unique(np.append(cells, rng.integers((y1 - y0) * (x1 - x0))))
        vals = rng.uniform(2.0, 60.0, size=n)
        if name == "clamps" and i == 1:
            vals = rng.uniform(0.004, 0.02, size=n)   # a ratio near 1e-3: predictions clamp at 1e-3 after scaling
        if name == "clamps" and i == 0:
            vals = rng.uniform(60.0, 79.0, size=n)    # a large ratio: predictions clamp at 80 after scaling
        if n >= 4:
            vals[1] = vals[0]                         # ties, also around the median
            vals[n // 2] = vals[(n - 1) // 2]
        g[y0 + cells // (x1 - x0), x0 + cells % (x1 - x0)] = vals.astype(g.dtype)
        gts.append(g)

    def disparity():
        d = rng.random((B, 1, h, w))
        d = np.where(rng.random((B, 1, h, w)) < 0.4, np.round(d * 8) / 8, d)   # plateaus: tied predictions
        if name == "clamps":   # min_depth 5e-4: the depth runs from 100 (disparity 0) down to 5e-4 (disparity 1)
            d = d ** 3 * 0.01
            d[:, 0, 1, 0:2] = 0.0      # depth 100 -> clamped at 80
            d[:, 0, 2, 3:5] = 1.0      # depth 5e-4 -> clamped at 1e-3
        if name == "ulps6x10":
            # same size: the taps are (1, 0), a prediction is the depth of its own pixel.  Disparities two ulp apart from
            # ULPS_BASE give distinct depths within 116 float32 values below 9.99901, which share their top 24 bits: only
            # the select's last 8-bit pass tells them apart.  The third image's are all equal.
            steps = np.stack([2 * rng.permutation(h * w) if i < 2 else np.zeros(h * w, np.int64) for i in range(B)])
            return torch.from_numpy((ULPS_BASE.view(np.int32) + steps.astype(np.int32)).view(np.float32).reshape(B, 1, h, w))
        return torch.from_numpy(d.astype(np.float32))

    disp, mono = disparity(), disparity()
    m = (rng.random((B, 1, mh, mw)) < 0.45).astype(np.float64)
    m = m * rng.choice([1.0, 0.25, 255.0 if mdt == "u1" else 2.5], size=m.shape)
    if mh * mw == 1:
        m[...] = 1.0
    if B >= 2 or name == "nodoj":
        m[min(1, B - 1)] = 0.0
    if B == 3:
        m[2] = 1.0
    mask = torch.from_numpy(np.floor(m).astype(np.uint8) if mdt == "u1" else m.astype(np.float32))
    return {"name": name, "split": split, "gt": gts, "disp": disp, "mono_disp": mono, "doj_mask": mask, "min_depth": dmin,
            "max_depth": dmax}


def admissible(c, tol=1e-4):
    """in both float32 forms of the resize, so that neither ATen's bits nor the written-out ones can flip a comparison"""
    return all(r["margin"] > tol for which in ("student", "mono") for rs in ("aten", "explicit")
               for r in evaluate_case(c, which, resize=rs))


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, "dyn_eval_%s.npz" % name), allow_pickle=False)
    return {k: z[k] for k in z.files}


def case_of_golden(z):
    n = int(z["n_images"])
    return {"name": str(z["name"]), "split": str(z["eval_split"]), "gt": [z["in:gt/%d" % i] for i in range(n)],
            "disp": torch.from_numpy(z["in:disp"]), "mono_disp": torch.from_numpy(z["in:mono_disp"]),
            "doj_mask": torch.from_numpy(z["in:doj_mask"]), "min_depth": float(z["min_depth"]), "max_depth": float(z["max_depth"])}
