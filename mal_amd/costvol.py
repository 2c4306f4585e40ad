"""ManyDepth's cost volume as MAL's student encoder builds it:
``ResnetEncoderMatching.match_features`` (manydepth/networks/resnet_encoder.py:152-233) and the lines of its
``forward`` that turn the volume into ``lowest_cost`` / ``confidence_mask`` (:296-312), as two HIP launches
(``mal_cost_volume``) instead of a Python loop over the batch with 96-fold feature replication.  Forward only,
as upstream (``torch.no_grad()``).  The kernels read the encoder's own NCHW feature maps.

``match_features_dynamic`` / ``cost_volume_outputs_dynamic``: DynamicDepth's occlusion-aware variant
(dynamicdepth/networks/resnet_encoder.py:148-249, ``mal_cost_volume_dyn``).
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import ops


# The input preparation of both routes, in the two halves between which the dynamic route handles its images and aug_mask
# (so that each route reports its refusals in the order it always did).
def _features(current_feats, lookup_feats):
    """-> (cur, look, (B, F, C, h, w)): the feature shape check, then both maps as contiguous float32 device tensors"""
    B, C, h, w = current_feats.shape
    if lookup_feats.dim() != 5 or lookup_feats.shape[0] != B or tuple(lookup_feats.shape[2:]) != (C, h, w):
        raise L.MalError("lookup_feats must be (B,F,C,h,w) matching current_feats (B,C,h,w)")
    cur = ops._req(current_feats.detach(), "current_feats")
    look = ops._req(lookup_feats.detach(), "lookup_feats")
    return cur, look, (B, look.shape[1], C, h, w)


def _geometry(dev, depth_bins, relative_poses, K, invK, B, F_):
    """-> (bins (D), poses (B,F,16), K (B,16), invK (B,16)) on the device"""
    bins = torch.as_tensor(depth_bins, dtype=torch.float32).to(dev).contiguous().reshape(-1)
    poses = ops._req(relative_poses.detach().reshape(B, F_, 16).contiguous(), "relative_poses")
    Kc, iKc = ops._req(K.detach().reshape(B, 16).contiguous(), "K"), ops._req(invK.detach().reshape(B, 16).contiguous(), "invK")
    return bins, poses, Kc, iKc


def _outputs(dev, B, D, h, w, want):
    """(cost volume, missing, masked, lowest_cost, confidence): the volume always, the others where ``want`` asks."""
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    return (new(B, D, h, w), new(B, D, h, w) if want["missing"] else None, new(B, D, h, w) if want["masked"] else None,
            new(B, h, w) if want["lowest"] else None, new(B, h, w) if want["confidence"] else None)


def _run(current_feats, lookup_feats, relative_poses, K, invK, depth_bins, set_missing_to_max, want):
    cur, look, (B, F_, C, h, w) = _features(current_feats, lookup_feats)
    bins, poses, Kc, iKc = _geometry(cur.device, depth_bins, relative_poses, K, invK, B, F_)
    D = bins.numel()
    if L.load().mal_costvol_channel_last():  # first formulation (mal_set_option("costvol_impl", 0)): relayout
        cl = cur.permute(0, 2, 3, 1).contiguous()
        ll = look.permute(0, 1, 3, 4, 2).contiguous()
    else:                                    # default: the kernels read the encoder's own (B,C,h,w) layout
        cl, ll = cur, look
    outs = _outputs(cur.device, B, D, h, w, want)
    p = ops._p
    L.check(L.load().mal_cost_volume(p(cl), p(ll), p(poses), p(Kc), p(iKc), p(bins), B, F_, C, D, h, w, 1e-7,
                                     1 if set_missing_to_max else 0, *[p(o) for o in outs], ops._stream()), "mal_cost_volume")
    return outs


def match_features(current_feats, lookup_feats, relative_poses, K, invK, depth_bins, set_missing_to_max=True):
    """resnet_encoder.py:152-233 -> (cost_volume (B,D,h,w), missing_mask (B,D,h,w)).  ``depth_bins``: the D depth
    hypotheses (``self.depth_bins`` upstream, from ``compute_depth_bins``)."""
    cv, miss, _, _, _ = _run(current_feats, lookup_feats, relative_poses, K, invK, depth_bins, set_missing_to_max,
                             dict(missing=True, masked=False, lowest=False, confidence=False))
    return cv, miss


def cost_volume_outputs(current_feats, lookup_feats, relative_poses, K, invK, depth_bins, set_missing_to_max=True):
    """match_features + :299-312 of the encoder's forward in the same two launches ->
    (cost_volume x confidence (B,D,h,w), lowest_cost (B,h,w), confidence_mask (B,h,w))."""
    _, _, masked, low, conf = _run(current_feats, lookup_feats, relative_poses, K, invK, depth_bins, set_missing_to_max,
                                   dict(missing=False, masked=True, lowest=True, confidence=True))
    return masked, low, conf


# ------------------------------------------------------------------ DynamicDepth's occlusion-aware variant
def _run_dynamic(current_feats, lookup_feats, relative_poses, K, invK, lookup_images, depth_bins, cv_min, aug_mask, set_1,
                 pool, pool_r, pool_th, set_missing_to_max, want):
    if int(pool_r) > 2 or int(pool_r) < 0:
        raise L.MalError("--cv_pool_radius %d: the pooled fill supports a radius of 0..2 (a wider window leaves the image "
                         "around the pixels that carry a cost)" % int(pool_r))
    cur, look, (B, F_, C, h, w) = _features(current_feats, lookup_feats)
    dev = cur.device
    occ = bool(set_1) or bool(pool)
    imgs, H, W = None, 0, 0
    if lookup_images is not None:
        imgs = ops._req(lookup_images.detach(), "lookup_images")
        if imgs.dim() == 5:  # forward's (B,F,3,H,W) before its reshape (:292)
            imgs = imgs.reshape(-1, *imgs.shape[2:])
        if imgs.dim() != 4 or imgs.shape[0] != B * F_ or imgs.shape[1] != 3:
            raise L.MalError("lookup_images must be (B*F,3,H,W) for lookup_feats (B,F,C,h,w)")
        H, W = int(imgs.shape[2]), int(imgs.shape[3])
    elif occ:
        raise L.MalError("set_1 / pool read the occlusions from lookup_images")
    aug = None
    if aug_mask is not None:
        aug = ops._req(aug_mask.detach(), "aug_mask")
        aug = aug.reshape(B, -1)[:, 0].contiguous()  # upstream reads aug_mask[b][0][0][0] (:192)
    bins, poses, Kc, iKc = _geometry(dev, depth_bins, relative_poses, K, invK, B, F_)
    D = bins.numel()
    lib = L.load()
    ws = None
    if occ:
        need = lib.mal_cost_volume_dyn_workspace_bytes(B, F_, D, h, w)
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    outs = _outputs(dev, B, D, h, w, want)
    p = ops._p
    L.check(lib.mal_cost_volume_dyn(p(cur), p(look), p(poses), p(Kc), p(iKc), p(bins), B, F_, C, D, h, w, 1e-7,
                                    1 if set_missing_to_max else 0, p(imgs), H, W, p(aug), int(bool(cv_min)),
                                    int(bool(set_1)), int(bool(pool)), int(pool_r), float(pool_th), *[p(o) for o in outs],
                                    p(ws), ws.numel() if ws is not None else 0, ops._stream()),
            "mal_cost_volume_dyn")
    return outs


def match_features_dynamic(current_feats, lookup_feats, relative_poses, K, invK, lookup_images, depth_bins, cv_min=True,
                           aug_mask=None, set_1=False, pool=False, pool_r=2, pool_th=0.4, set_missing_to_max=True):
    """dynamicdepth/networks/resnet_encoder.py:148-249 -> (cost_volume (B,D,h,w), missing_mask (B,D,h,w)).
    ``lookup_images`` (B*F,3,H,W) or (B,F,3,H,W): the images the lookup features come from, whose black pixels (channel
    sum < 0.15) are the holes ``rigid_warp.warp_dynamic_objects`` leaves.  ``aug_mask`` (B,...) or None (= zeros): a
    sample with a non-zero first element gets no occlusion handling; it is read on the device, as is the all-zero pose
    of a missing frame, so the call can be captured.  Upstream's ``occ[b]`` indexing of the flattened (B*F) occlusion
    images is kept."""
    cv, miss, _, _, _ = _run_dynamic(current_feats, lookup_feats, relative_poses, K, invK, lookup_images, depth_bins, cv_min,
                                     aug_mask, set_1, pool, pool_r, pool_th, set_missing_to_max,
                                     dict(missing=True, masked=False, lowest=False, confidence=False))
    return cv, miss


def cost_volume_outputs_dynamic(current_feats, lookup_feats, relative_poses, K, invK, lookup_images, depth_bins, cv_min=True,
                                aug_mask=None, set_1=False, pool=False, pool_r=2, pool_th=0.4, set_missing_to_max=True):
    """match_features_dynamic + :302-312 of the encoder's forward in the same call ->
    (cost_volume x confidence (B,D,h,w), lowest_cost (B,h,w), confidence_mask (B,h,w))."""
    _, _, masked, low, conf = _run_dynamic(current_feats, lookup_feats, relative_poses, K, invK, lookup_images, depth_bins,
                                           cv_min, aug_mask, set_1, pool, pool_r, pool_th, set_missing_to_max,
                                           dict(missing=False, masked=True, lowest=True, confidence=True))
    return masked, low, conf
