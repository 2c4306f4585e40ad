"""CPU checker for ``mal_amd.instances`` (``mal_instances``): the inference tail of mask2former/maskformer_model.py
(:219-227 the x4 bilinear upsample, :344-380 ``instance_inference``) in fp64 numpy, with the order this library defines.

TEST INFRASTRUCTURE ONLY.  Three things:

``upsample_x4``   ATen's rule for ``F.interpolate(mode="bilinear", align_corners=False)`` at scale 1/4, cropped: for an
                  output index o, source s = max((o + 0.5)/4 - 0.5, 0), i0 = floor(s), i1 = min(i0 + 1, n - 1), weight
                  s - i0 on i1.  Interior weights are 1/8 3/8 5/8 7/8; the first two outputs have weight 0 on tap 1, the
                  last two have both taps on the last texel.
``checker``       softmax in fp64, the T largest of the Q*K values in DESCENDING score with ties by ASCENDING flat index
                  q*K + c (upstream's topk(sorted=False) leaves the order open), the thing filter after the top-k,
                  mask = upsampled value > 0 (strictly), mask_score = sum of sigmoid over the set pixels / (count + 1e-6),
                  score = cls_score * mask_score.
``torch_tail``    upstream's tail restated with torch operators in fp32, on whatever device its inputs live: the path the
                  library call replaces, for the device tests and scripts/bench_instances.py.

tests/test_instances_host.py holds the checker to the reference's own outputs (tests/golden/instances_*.npz, written by
scripts/gen_golden_instances.py)."""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
#        tag  Q    K  h  w   H   W   T
CASES = {"a": (3, 1, 1, 1, 4, 4, 3),
         "b": (4, 3, 2, 3, 6, 10, 8),
         "c": (10, 8, 6, 10, 24, 40, 10),
         "d": (10, 8, 6, 10, 21, 37, 10),
         "e": (6, 8, 6, 10, 24, 40, 6),
         "f": (130, 2, 3, 5, 12, 20, 128)}
MASK_UNIT = 256  # fixtures store the mask logits as int16 multiples of 1/256


def taps(n_out, n_in):
    """(i0, i1, weight on i1) of the outputs 0..n_out-1 over n_in texels, 4(n_in - 1) < n_out <= 4 n_in"""
    assert 4 * (n_in - 1) < n_out <= 4 * n_in
    s = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) / 4.0 - 0.5, 0.0)
    i0 = np.floor(s).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, s - i0


def upsample_x4(planes, H, W):
    """(..., h, w) -> (..., H, W) float64 by the rule above"""
    x = np.asarray(planes, dtype=np.float64)
    y0, y1, wy = taps(H, x.shape[-2])
    x0, x1, wx = taps(W, x.shape[-1])
    rows = x[..., y0, :] * (1.0 - wy)[:, None] + x[..., y1, :] * wy[:, None]
    return rows[..., x0] * (1.0 - wx) + rows[..., x1] * wx


def tap_magnitude(planes, H, W):
    """largest magnitude among the four taps of every output pixel, (..., H, W)"""
    a = np.abs(np.asarray(planes, dtype=np.float64))
    y0, y1, _ = taps(H, a.shape[-2])
    x0, x1, _ = taps(W, a.shape[-1])
    rows = np.maximum(a[..., y0, :], a[..., y1, :])
    return np.maximum(rows[..., x0], rows[..., x1])


def class_scores(logits):
    """(Q, K+1) -> (Q*K,) fp64 softmax without the last column, flattened"""
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True))[:, :-1].reshape(-1)


def select(scores, T):
    """the T largest in descending score, ties by ascending index"""
    order = np.lexsort((np.arange(len(scores)), -scores))
    return order[:T]


def class_scores_fp32(logits):
    """the fp64 softmax rounded ONCE to float32 (IEEE: to nearest even, denormals kept): what the kernel orders by"""
    return class_scores(logits).astype(np.float32)


def select_fp32(logits, T):
    """the library's rule where fp64 and fp32 part ways (probabilities that underflow): the T largest in descending
    ROUNDED score, ties by ascending flat index"""
    return select(class_scores_fp32(logits).astype(np.float64), T)


def checker(logits, planes, H, W, T, thing=None, fp32_rule=False):
    """one image.  logits (Q,K+1), planes (Q,h,w), thing: K-entry table or None -> dict: flat (the selected flat indices
    q*K + c after the filter, in order), query, classes, masks (n,H,W) bool, cls_score, mask_score, score (fp64),
    flat_topk (before the filter), margin_cut (relative gap between the T-th and the (T+1)-th class score, inf without a
    (T+1)-th) and margin_sel (smallest relative gap between two selected ones).  ``fp32_rule``: the class scores are the
    rounded ones of ``class_scores_fp32`` and the selection is ``select_fp32``."""
    Q, K = logits.shape[0], logits.shape[1] - 1
    s = class_scores_fp32(logits).astype(np.float64) if fp32_rule else class_scores(logits)
    flat_topk = select(s, T)
    ordered = np.sort(s)[::-1]
    rel = lambda a, b: abs(a - b) / max(abs(a), abs(b), 1e-300)
    margin_cut = rel(ordered[T - 1], ordered[T]) if T < len(s) else np.inf
    margin_sel = min([rel(ordered[k], ordered[k + 1]) for k in range(T - 1)] or [np.inf])
    flat = flat_topk
    if thing is not None:
        flat = flat[np.asarray(thing, dtype=bool)[flat % K]]
    query, classes = flat // K, flat % K
    v = upsample_x4(np.asarray(planes, dtype=np.float64)[query], H, W) if len(flat) else np.zeros((0, H, W))
    masks = v > 0
    count = masks.reshape(len(flat), H * W).sum(1).astype(np.float64)
    sig = np.where(masks, 1.0 / (1.0 + np.exp(-np.where(masks, v, 0.0))), 0.0).reshape(len(flat), H * W).sum(1)
    mask_score = sig / (count + 1e-6)
    cls_score = s[flat]
    return {"flat": flat, "flat_topk": flat_topk, "query": query, "classes": classes, "masks": masks, "cls_score": cls_score,
            "mask_score": mask_score, "score": cls_score * mask_score, "margin_cut": margin_cut, "margin_sel": margin_sel}


def load_case(tag):
    """fixture -> dict: Q K h w H W T, logits (Q,K+1) fp32, planes (Q,h,w) fp32 (multiples of 1/256), thing (K bool or
    None); the reference's outputs in ITS order: ref_masks (n,H,W) bool, ref_scores fp32, ref_classes, ref_flat; the
    checker's fp64 cls_score / mask_score / score in the defined order; ref_dist (3): the reference's own fp32 relative
    distance from them; margins (3): cut, selected, distance of a score from 0.9."""
    z = np.load(os.path.join(GOLDEN, "instances_%s.npz" % tag))
    Q, K, h, w, H, W, T = (int(v) for v in z["dims"])
    d = {"Q": Q, "K": K, "h": h, "w": w, "H": H, "W": W, "T": T}
    d["logits"] = z["logits"].astype(np.float32)
    d["planes"] = (z["planes_q8"].astype(np.float32) / MASK_UNIT).reshape(Q, h, w)
    d["thing"] = z["thing"].astype(bool) if z["thing"].size else None
    n = len(z["ref_flat"])
    d["ref_masks"] = np.unpackbits(z["ref_masks_bits"], count=n * H * W).astype(bool).reshape(n, H, W)
    for k in ("ref_scores", "ref_classes", "ref_flat", "cls_score", "mask_score", "score", "ref_dist", "margins"):
        d[k] = z[k]
    return d


def rel_dist(x, x64):
    """largest |x - x64| / |x64|; where x64 is 0 (an empty mask) x must be 0 as well, else inf"""
    x, x64 = np.asarray(x, dtype=np.float64), np.asarray(x64, dtype=np.float64)
    if x.size == 0:
        return 0.0
    zero = x64 == 0
    if np.any(x[zero] != 0):
        return np.inf
    return float((np.abs(x - x64)[~zero] / np.abs(x64[~zero])).max()) if (~zero).any() else 0.0


def torch_tail(pred_logits, pred_masks, H, W, T, thing=None):
    """upstream's tail for a batch, fp32 torch operators on the inputs' device: maskformer_model.py:222-227 (the padded
    size is 4 (h, w)), the crop, then :344-380 per image.  -> list of dicts: flat (as topk returned them, filtered),
    masks (n,H,W) bool, scores, classes, cls_score, mask_score."""
    h, w = pred_masks.shape[-2:]
    up = F.interpolate(pred_masks, size=(4 * h, 4 * w), mode="bilinear", align_corners=False)[..., :H, :W]
    out = []
    for mask_cls, mask_pred in zip(pred_logits, up):
        K = mask_cls.shape[-1] - 1
        scores = F.softmax(mask_cls, dim=-1)[:, :-1]
        scores_per_image, topk_indices = scores.flatten(0, 1).topk(T, sorted=False)
        if thing is not None:
            keep = torch.as_tensor(thing, dtype=torch.bool, device=mask_cls.device)[topk_indices % K]
            scores_per_image, topk_indices = scores_per_image[keep], topk_indices[keep]
        labels = topk_indices % K
        mask_pred = mask_pred[torch.div(topk_indices, K, rounding_mode="trunc")]
        masks = (mask_pred > 0).float()
        mask_scores = (mask_pred.sigmoid().flatten(1) * masks.flatten(1)).sum(1) / (masks.flatten(1).sum(1) + 1e-6)
        out.append({"flat": topk_indices, "masks": masks.bool(), "scores": scores_per_image * mask_scores, "classes": labels,
                    "cls_score": scores_per_image, "mask_score": mask_scores})
    return out


GENERAL_SEED = 20  # confirmed on the CPU by tests/test_instances_host.py::test_general_seed_on_the_cpu


def general_inputs(seed=GENERAL_SEED, Q=100, K=8, h=48, w=160):
    """general fp32 inputs: N(0, 4) mask logits (standard deviation 2, nothing dyadic about them) and N(0, 4) class logits"""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((Q, K + 1)) * 2.0).astype(np.float32)
    planes = (rng.standard_normal((Q, h, w)) * 2.0).astype(np.float32)
    return logits, planes


def band_report(masks, planes, H, W, width=4.0):
    """masks (n,H,W) bool of the planes (n,h,w) against the fp64 rule -> (pixels that differ outside the band, pixels that
    differ, pixels inside the band); the band is |fp64 value| <= width * 2^-23 * (largest tap magnitude): the fp32
    rounding of three multiply-adds"""
    v = upsample_x4(planes, H, W)
    inside = np.abs(v) <= width * 2.0 ** -23 * tap_magnitude(planes, H, W)
    differ = np.asarray(masks, dtype=bool) != (v > 0)
    return int((differ & ~inside).sum()), int(differ.sum()), int(inside.sum())
