"""DynamicDepth's occlusion-aware forward warp (``dynamicdepth/rigid_warp.py:534-597``) and the warped-object composition
its trainer builds on it (``dynamicdepth/trainer.py:493-534``), on the HIP library (``mal_forward_warp`` /
``mal_inverse_warp``, include/mal_hip.h, mal_amd/csrc/mal_fwarp.hip).

Upstream's ``rigid_warp.py`` imports ``coalesce`` from ``torch_sparse`` (:7), a third-party package of compiled CUDA
kernels, so ``dynamicdepth/trainer.py:17`` does not import without it.  The z-buffer ``coalesce(..., op='max')`` builds is
an integer ``atomicMax`` here; see the kernel file for the arithmetic.

``forward_warp(img, depth, pose, intrinsics, upscale=None, rotation_mode='euler', padding_mode='zeros')``
    upstream's signature, argument shapes and return tuple ``(img_w * valid, depth_w * valid, valid)``.
``inverse_warp(img, depth, pose, intrinsics)``
    ``rigid_warp.py:337-373`` for Euler angles and zero padding.
``warp_dynamic_objects(...)``
    the whole block of ``trainer.py:493-534`` in two library calls, with no host read.

Forward only: upstream runs all of it under ``torch.no_grad()`` (``trainer.py:494``); a tensor that requires grad is
refused.  There is no CPU path: a CPU tensor or a missing library raises ``MalError``.
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import ops

NO_BACKWARD = ("mal_amd.rigid_warp is forward only: upstream warps the dynamic objects under torch.no_grad() "
               "(dynamicdepth/trainer.py:494) from detached clones, so no gradient is ever taken through it")


def _refuse_grad(*tensors):
    if any(torch.is_tensor(t) and t.requires_grad for t in tensors):
        raise NotImplementedError(NO_BACKWARD + "; pass detached tensors")


def _check_hw(H, W, what):
    if H < 2 or W < 2:
        raise L.MalError("%s: the image must be at least 2x2 (upstream divides by W - 1 and H - 1), got %dx%d" % (what, H, W))


def _shapes(img, depth, intrinsics, what):
    if img.dim() != 4 or depth.dim() != 4 or depth.shape[1] != 1 or intrinsics.dim() != 3:
        raise L.MalError("%s: expected img (B,C,H,W), depth (B,1,H,W) and intrinsics (B,3,3), got %s, %s, %s"
                         % (what, tuple(img.shape), tuple(depth.shape), tuple(intrinsics.shape)))
    _check_hw(img.shape[2], img.shape[3], what)


def forward_warp(img, depth, pose, intrinsics, upscale=None, rotation_mode='euler', padding_mode='zeros'):
    """img (B,C,H,W), depth (B,1,H,W) of that same image, pose (B,3,4) from it to the target view, intrinsics (B,3,3)
    -> (img_w * valid (B,C,H,W), depth_w * valid (B,1,H,W), valid (B,1,H,W)).  ``rotation_mode`` and ``padding_mode`` are
    accepted and ignored, as upstream ignores them (it passes neither on to ``inverse_warp``, :591)."""
    if upscale is None:
        raise ValueError("forward_warp: upscale is required (upstream's default None fails inside F.interpolate); "
                         "DynamicDepth passes upscale=3")
    _shapes(img, depth, intrinsics, "forward_warp")
    _refuse_grad(img, depth, pose, intrinsics)
    img_w, depth_w, valid, _ = ops.forward_warp(img, depth[:, 0], [pose], intrinsics, upscale)
    return img_w[0], depth_w[0].unsqueeze(1), valid[0].unsqueeze(1)


def inverse_warp(img, depth, pose, intrinsics, rotation_mode='euler', padding_mode='zeros'):
    """img (B,C,H,W), depth (B,H,W) of the target view, pose (B,6) = (tx, ty, tz, rx, ry, rz) from target to source,
    intrinsics (B,3,3) -> (projected_img (B,C,H,W), valid_points (B,H,W) bool).  Euler angles and zero padding only."""
    if rotation_mode != 'euler':
        raise NotImplementedError("inverse_warp: rotation_mode=%r is not built; only 'euler' is (forward_warp uses no other)"
                                  % (rotation_mode,))
    if padding_mode != 'zeros':
        raise NotImplementedError("inverse_warp: padding_mode=%r is not built; only 'zeros' is (forward_warp uses no other)"
                                  % (padding_mode,))
    if img.dim() != 4 or depth.dim() != 3:
        raise L.MalError("inverse_warp: expected img (B,C,H,W) and depth (B,H,W), got %s, %s" % (tuple(img.shape), tuple(depth.shape)))
    _check_hw(img.shape[2], img.shape[3], "inverse_warp")
    _refuse_grad(img, depth, pose, intrinsics)
    return ops.inverse_warp(img, depth, pose, intrinsics)


def _byte_mask(m, name):
    """a (B,1,H,W) or (B,H,W) mask as upstream compares it (``== 1``) -> (B,H,W) bytes on the device"""
    if m is None:
        return None
    if m.dim() == 4:
        m = m[:, 0]
    return (m == 1).view(torch.uint8) if m.dtype != torch.uint8 else m


def warp_dynamic_objects(color, teacher_depth, intrinsics, doj_mask, pose_m1, color_m1, doj_mask_m1, pose_p1=None, color_p1=None,
                         doj_mask_p1=None, color_aug=None, lookup_frame=None, augmentation_mask=None, upscale=3,
                         no_reproj_doj=False, no_teacher_warp=False):
    """``dynamicdepth/trainer.py:493-534``: the target frame's dynamic objects (``color`` with everything outside
    ``doj_mask`` set to 0) are forward-warped with the teacher's depth into the neighbouring frames and pasted over them.

    ``color`` (B,C,H,W), ``teacher_depth`` (B,1,H,W), ``intrinsics`` (B,3,3), ``doj_mask`` / ``doj_mask_m1`` / ``doj_mask_p1``
    (B,1,H,W), poses (B,3,4).  ``color_m1`` and ``color_p1`` (the latter with ``pose_p1``, training only, :523) are composed
    IN PLACE and must be contiguous.  With ``color_aug`` (the augmented target) and ``lookup_frame`` (B,C,H,W, upstream's
    ``lookup_frames[:, 0]``), the lookup frame of every sample whose ``augmentation_mask[b, 0, 0, 0]`` is 0 is composed in
    place from the warped augmented objects (:513-521); the selector is read on the device, so nothing here synchronises.
    ``no_reproj_doj``: the pasted pixels are 0 (:509-510), in the two neighbouring frames only, as upstream has it.
    ``no_teacher_warp``: also returns clones of the frames before composition, as upstream stores them (:505, :528 -- where
    upstream stores the ALREADY COMPOSED frame -1 under the key of frame +1; kept).

    Two library calls: the two poses share image and depth (one call, poses on the grid's z axis); the augmented image
    is the second.  -> dict with ``img_w_m1``, ``img_w_p1``, ``imgaug_w_m1`` (those that were computed) and, with
    ``no_teacher_warp``, ``ori_color_m1`` / ``ori_color_p1``."""
    _shapes(color, teacher_depth, intrinsics, "warp_dynamic_objects")
    _refuse_grad(color, teacher_depth, intrinsics, pose_m1, pose_p1, color_m1, color_p1, color_aug, lookup_frame)
    out = {}
    keep = doj_mask != 0                                       # :501 zeroes where the mask == 0
    depth = teacher_depth[:, 0]
    tgt = color * keep.to(color.dtype)                         # :497,501
    poses, dst, masks = [pose_m1], [color_m1], [_byte_mask(doj_mask_m1, "doj_mask_m1")]
    if no_teacher_warp:
        out["ori_color_m1"] = color_m1.detach().clone()        # :505
    if pose_p1 is not None:
        poses.append(pose_p1)
        dst.append(color_p1)
        masks.append(_byte_mask(doj_mask_p1, "doj_mask_p1"))
    img_w, _, _, _ = ops.forward_warp(tgt, depth, poses, intrinsics, upscale, dst=dst, masks=masks, no_reproj=no_reproj_doj)
    out["img_w_m1"] = img_w[0]
    if pose_p1 is not None:
        out["img_w_p1"] = img_w[1]
        if no_teacher_warp:
            out["ori_color_p1"] = color_m1.detach().clone()    # :528
    if color_aug is not None:
        if lookup_frame is None or augmentation_mask is None:
            raise L.MalError("warp_dynamic_objects: color_aug needs lookup_frame and augmentation_mask")
        select = (augmentation_mask.reshape(augmentation_mask.shape[0], -1)[:, 0] == 0).view(torch.uint8)  # :513
        tgt_aug = color_aug * keep.to(color_aug.dtype)                                                      # :515-516
        aug_w, _, _, _ = ops.forward_warp(tgt_aug, depth, [pose_m1], intrinsics, upscale, dst=[lookup_frame], masks=[masks[0]],
                                          select=select)
        out["imgaug_w_m1"] = aug_w[0]
    return out
