"""The temporal-hint producer's instance matcher on the device: ``manydepth/matcher.py:63-245`` (``HungarianMatcher``)
as three HIP launches (``mal_match``, include/mal_hip.h) instead of two dense fp32 einsums over sigmoid copies of the
masks, two ``.cpu()`` syncs, two ``scipy.optimize.linear_sum_assignment`` calls, a Python set intersection and two
host-to-device copies per confident sample.  Same constructor and call signature as upstream, so
``trainer.matcher = mal_amd.matcher.HungarianMatcher()`` replaces upstream's import; neither detectron2 nor scipy is
needed.

What is the same: the two cost matrices (class term + dice term of the BINARY masks Mask2Former emits,
``mask2former/maskformer_model.py:371``; ``cost_mask`` is accepted and unused, as upstream) and the optimal assignment of
each, hence the SET of matched (row of ``instances_n``, row of ``instances_m``) pairs wherever each optimum is unique.

What differs: the ORDER of the pairs.  Upstream emits them in CPython's iteration order of ``set(idx_0) & set(idx_1)``;
here they come in ascending index of the target instance.  The order matters only where shifted instances overlap:
``fill_dynamic_obj`` sums the overlapping copies in fp32 in that order.  Between tied optima the choice is not upstream's
either (scipy's own tie-break is not reproduced).
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn

from . import _lib as L
from . import ops


def _masks(inst, what):
    m = inst.pred_masks
    if not torch.is_tensor(m) or not m.is_cuda:
        raise L.MalError("HungarianMatcher: %s.pred_masks must be a device tensor (there is no CPU path)" % what)
    if m.dim() != 3:
        raise L.MalError("HungarianMatcher: %s.pred_masks must be (N,H,W)" % what)
    if m.dtype == torch.bool:
        return m.contiguous().view(torch.uint8), L.MATCH_U8
    if m.dtype == torch.uint8:
        return m.contiguous(), L.MATCH_U8
    return m.contiguous().float(), L.MATCH_F32  # upstream's .float() (matcher.py:116-118)


def _classes(inst, what, n, dev):
    c = inst.pred_classes
    if not torch.is_tensor(c) or not c.is_cuda:
        raise L.MalError("HungarianMatcher: %s.pred_classes must be a device tensor (there is no CPU path)" % what)
    if c.numel() != n:
        raise L.MalError("HungarianMatcher: %s has %d masks and %d classes" % (what, n, c.numel()))
    return c.to(device=dev, dtype=torch.int64).contiguous()


class HungarianMatcher(nn.Module):
    """Upstream's matcher (manydepth/matcher.py:63).  ``forward(instances_n, instances_m, instances_0)`` reads only
    ``.pred_classes``, ``.pred_masks`` and ``len()`` of its arguments (any Instances-like object) and returns
    ``(slice_n, slice_m)``: two int64 DEVICE tensors, views of a 128-slot buffer allocated per call (a producer call holds
    the selections of several samples until its kernels run), which ``dyn_utils.image_synthesis`` hands to its kernels as
    they are.  Pairs come in ascending target index, not in upstream's set-iteration order (module docstring).  One
    host readback per call: the 16-byte result block (count, non-binary flag).  ``last_costs``: the (C1, C2) of the last
    call, fp32 device tensors."""

    def __init__(self, cost_class: float = 1, cost_mask: float = 1, cost_dice: float = 1, ins_threshold: float = 0.5):
        super().__init__()
        self.cost_class = cost_class
        self.cost_mask = cost_mask
        self.cost_dice = cost_dice
        self.ins_threshold = ins_threshold
        assert cost_class != 0 or cost_mask != 0 or cost_dice != 0, "all costs cant be 0"
        self.last_costs = None

    @torch.no_grad()
    def memory_efficient_forward(self, instances_n, instances_m, instances_0):
        sets = (("instances_n", instances_n), ("instances_m", instances_m), ("instances_0", instances_0))
        masks, kinds = zip(*(_masks(inst, what) for what, inst in sets))
        dev = masks[0].device
        nums = [len(inst) for _, inst in sets]
        H, W = masks[0].shape[1:]
        for (what, _), m, n in zip(sets, masks, nums):
            if m.device != dev or tuple(m.shape) != (n, H, W):
                raise L.MalError("HungarianMatcher: %s.pred_masks is %s on %s, expected %s on %s"
                                 % (what, tuple(m.shape), m.device, (n, H, W), dev))
            if n > L.MATCH_MAX:
                raise L.MalError("HungarianMatcher: %s holds %d instances, at most %d are supported" % (what, n, L.MATCH_MAX))
        if H * W == 0:
            raise L.MalError("HungarianMatcher: empty masks")
        classes = [_classes(inst, what, n, dev) for (what, inst), n in zip(sets, nums)]
        lib, p = L.load(), ops._p
        with torch.cuda.device(dev):
            # slice_n, slice_m (128 slots each) and the result block in one allocation; the two matrices in another
            out = torch.empty(2 * L.MATCH_MAX + 2, dtype=torch.int64, device=dev)
            costs = torch.empty((nums[0] + nums[1]) * nums[2], dtype=torch.float32, device=dev)
            ws = torch.empty(int(lib.mal_match_workspace_bytes(nums[0], nums[1], nums[2], H, W)), dtype=torch.uint8, device=dev)
            C1, C2 = costs[:nums[0] * nums[2]].view(nums[0], nums[2]), costs[nums[0] * nums[2]:].view(nums[1], nums[2])
            slice_n, slice_m, result = out[:L.MATCH_MAX], out[L.MATCH_MAX:2 * L.MATCH_MAX], out[2 * L.MATCH_MAX:].view(torch.int32)
            a = L.MatchArgs()
            a.masks_n, a.masks_m, a.masks_0 = (p(m) if m.numel() else None for m in masks)
            a.kind_n, a.kind_m, a.kind_0 = kinds
            a.n_n, a.n_m, a.n_0, a.H, a.W = nums[0], nums[1], nums[2], H, W
            a.class_n, a.class_m, a.class_0 = (p(c) if c.numel() else None for c in classes)
            a.cost_class, a.cost_mask, a.cost_dice = float(self.cost_class), float(self.cost_mask), float(self.cost_dice)
            a.C1, a.C2 = (p(C1) if C1.numel() else None), (p(C2) if C2.numel() else None)
            a.slice_n, a.slice_m, a.result = p(slice_n), p(slice_m), p(result)
            a.ws, a.ws_bytes, a.stream = p(ws), ws.numel(), ops._stream()
            L.check(lib.mal_match(ctypes.byref(a)), "mal_match")
            count, non_binary = result[:2].tolist()  # the one readback
        if non_binary:
            raise L.MalError("HungarianMatcher: a float mask holds a value that is neither 0 nor 1; upstream matches the binary "
                             "masks of mask2former/maskformer_model.py:371 ((mask_pred > 0).float()) and the sigmoid of any "
                             "other value has no integer form here: pass the thresholded masks (or bool / uint8)")
        self.last_costs = (C1, C2)
        return slice_n[:count], slice_m[:count]

    @torch.no_grad()
    def forward(self, outputs1, outputs2, targets):
        return self.memory_efficient_forward(outputs1, outputs2, targets)

    def __repr__(self, _repr_indent=4):
        head = "Matcher " + self.__class__.__name__
        body = ["cost_class: {}".format(self.cost_class), "cost_mask: {}".format(self.cost_mask),
                "cost_dice: {}".format(self.cost_dice)]
        return "\n".join([head] + [" " * _repr_indent + line for line in body])
