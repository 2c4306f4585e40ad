"""The segmenter's inference tail on the device: ``mask2former/maskformer_model.py:219-227`` (the x4 bilinear upsample of
the mask logits) and ``:344-380`` (``MaskFormer.instance_inference``) as ONE library call for a whole batch
(``mal_instances``, include/mal_hip.h: three HIP launches) instead of an fp32 upsample of all Q planes, a softmax, a
top-k, a gather, a float threshold copy, a sigmoid copy, two full-size products and sums and a Python loop over the labels
per image.  The masks come out as bytes, what ``mal_amd.matcher.HungarianMatcher`` and ``dyn_utils.image_synthesis`` read;
no float mask is written.  detectron2 is not needed: ``Instances`` below is the slice of its class the producer touches.

What is the same as upstream: the selected (query, class) pairs, the masks (``upsampled logit > 0``), the scores
(class probability x mean sigmoid over the set pixels, to fp32 rounding).  What is defined here and open upstream
(``topk(sorted=False)``): the order, descending class probability with ties broken by ascending flat index q*K + c.

``InstanceSegmenter`` wraps a network that returns ``{"pred_logits", "pred_masks"}`` into the ``ins_model`` that
``dyn_utils.generate_instances`` calls.
"""
from __future__ import annotations

import ctypes

import torch
from torch import nn
from torch.nn import functional as F

from . import _lib as L
from . import ops


class Instances:
    """The slice of ``detectron2.structures.Instances`` that ``image_synthesis`` and the matcher touch: ``image_size``
    (H, W), ``pred_masks`` (n,H,W) uint8 on the device, ``scores`` (n) fp32, ``pred_classes`` (n) int64, ``len()`` and
    indexing by a bool mask, an index tensor, a slice or an int (which keeps the instance axis, as detectron2 does).
    ``extra``: further per-instance tensors that are indexed along (``query``, ``cls_score``, ``mask_score``)."""

    def __init__(self, image_size, pred_masks, scores, pred_classes, **extra):
        self.image_size = tuple(int(s) for s in image_size)
        self.pred_masks, self.scores, self.pred_classes = pred_masks, scores, pred_classes
        self._extra = dict(extra)
        n = len(pred_classes)
        for name, t in (("pred_masks", pred_masks), ("scores", scores)) + tuple(self._extra.items()):
            if len(t) != n:
                raise L.MalError("Instances: %s holds %d entries, pred_classes %d" % (name, len(t), n))

    def __getattr__(self, name):
        extra = self.__dict__.get("_extra", {})
        if name in extra:
            return extra[name]
        raise AttributeError("Instances has no field %r" % name)

    def __len__(self):
        return len(self.pred_classes)

    def __getitem__(self, item):
        if isinstance(item, int):
            if item >= len(self) or item < -len(self):
                raise IndexError("Instances index out of range")
            item = slice(item, None, len(self)) if item >= 0 else slice(item + len(self), None, len(self))
        elif torch.is_tensor(item):
            item = item.to(self.pred_classes.device)
        pick = lambda t: t[item]
        return Instances(self.image_size, pick(self.pred_masks), pick(self.scores), pick(self.pred_classes),
                         **{k: pick(v) for k, v in self._extra.items()})

    def __repr__(self):
        return "Instances(num_instances=%d, image_height=%d, image_width=%d)" % ((len(self),) + self.image_size)


def _thing_table(thing_classes, K, dev):
    if thing_classes is None:
        return None
    if torch.is_tensor(thing_classes) and thing_classes.dtype in (torch.bool, torch.uint8) and thing_classes.numel() == K:
        return thing_classes.to(device=dev, dtype=torch.uint8).contiguous()
    ids = [int(c) for c in (thing_classes.tolist() if torch.is_tensor(thing_classes) else thing_classes)]
    if any(c < 0 or c >= K for c in ids):
        raise L.MalError("instance_inference: thing_classes holds a class outside 0..%d" % (K - 1))
    table = torch.zeros(K, dtype=torch.uint8)
    if ids:
        table[torch.as_tensor(ids, dtype=torch.int64)] = 1
    return table.to(dev)


@torch.no_grad()
def instance_inference(pred_logits, pred_masks, image_size, topk=100, thing_classes=None):
    """(N,Q,K+1) class logits and (N,Q,h,w) mask logits -> a list of N ``{"instances": Instances}`` at ``image_size`` =
    (H, W), 4(h-1) < H <= 4h and likewise W: the crop of the x4 plane to the image.  ``topk``: upstream's
    ``test_topk_per_image``; ``thing_classes``: class ids to keep (or a K-entry bool / uint8 table), upstream's
    ``panoptic_on`` filter, applied after the top-k; None keeps every class.  One library call for the batch and one
    readback (the N counts); the per-image tensors are views of the batch outputs, trimmed to the image's count."""
    for name, t, dim in (("pred_logits", pred_logits, 3), ("pred_masks", pred_masks, 4)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise L.MalError("instance_inference: %s must be a device tensor (there is no CPU path)" % name)
        if t.dim() != dim:
            raise L.MalError("instance_inference: %s must have %d dimensions, got %s" % (name, dim, tuple(t.shape)))
    N, Q, K1 = pred_logits.shape
    K = K1 - 1
    if tuple(pred_masks.shape[:2]) != (N, Q) or pred_masks.device != pred_logits.device:
        raise L.MalError("instance_inference: pred_masks is %s on %s, expected (%d, %d, h, w) on %s"
                         % (tuple(pred_masks.shape), pred_masks.device, N, Q, pred_logits.device))
    h, w = pred_masks.shape[2:]
    H, W = (int(s) for s in image_size)
    topk = int(topk)
    dev = pred_logits.device
    lib, p = L.load(), ops._p
    ws_bytes = int(lib.mal_instances_workspace_bytes(N, Q, K, h, w, H, W, topk))
    if ws_bytes == 0:
        raise L.MalError("instance_inference: N=%d Q=%d K=%d %dx%d -> %dx%d topk=%d is not supported: the output must be the "
                         "crop of the x4 plane (4(h-1) < H <= 4h), 1 <= topk <= min(Q*K, %d) and Q*K <= 16384"
                         % (N, Q, K, h, w, H, W, topk, L.MATCH_MAX))
    logits, planes = ops._req(pred_logits, "pred_logits"), ops._req(pred_masks, "pred_masks")
    thing = _thing_table(thing_classes, K, dev)
    with torch.cuda.device(dev):
        masks = torch.empty((N, topk, H, W), dtype=torch.uint8, device=dev)
        classes = torch.empty((N, topk), dtype=torch.int64, device=dev)
        f32 = torch.empty((3, N, topk), dtype=torch.float32, device=dev)  # scores, cls_score, mask_score
        i32 = torch.empty(N * topk + N, dtype=torch.int32, device=dev)    # query, count
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        query, count = i32[:N * topk].view(N, topk), i32[N * topk:]
        a = L.InstancesArgs()
        a.pred_logits, a.pred_masks, a.thing = p(logits), p(planes), p(thing)
        a.N, a.Q, a.K, a.h, a.w, a.H, a.W, a.topk = N, Q, K, h, w, H, W, topk
        a.count, a.masks, a.scores, a.classes, a.query = p(count), p(masks), p(f32[0]), p(classes), p(query)
        a.cls_score, a.mask_score = p(f32[1]), p(f32[2])
        a.ws, a.ws_bytes, a.stream = p(ws), ws.numel(), ops._stream()
        L.check(lib.mal_instances(ctypes.byref(a)), "mal_instances")
        counts = count.tolist()  # the one readback
    return [{"instances": Instances((H, W), masks[n, :c], f32[0, n, :c], classes[n, :c], query=query[n, :c],
                                    cls_score=f32[1, n, :c], mask_score=f32[2, n, :c])} for n, c in enumerate(counts)]


class InstanceSegmenter(nn.Module):
    """The ``ins_model`` of ``dyn_utils.generate_instances``: ``forward(images)`` with (N,3,H,W) RGB in [0, 1] on the
    device -> a list of N ``{"instances": Instances}`` at (H, W).  ``net(padded) -> {"pred_logits": (N,Q,K+1),
    "pred_masks": (N,Q,H'/4,W'/4)}`` is the segmenter network (backbone + head); around it:
    upstream's input convention, BGR x 255 (manydepth/dyn_utils.py:175-179), ``(x - pixel_mean) / pixel_std`` and zero
    padding at the right and bottom to a multiple of ``size_divisibility`` (mask2former/maskformer_model.py:193-195), in
    plain torch operations, and ``instance_inference`` behind it."""

    def __init__(self, net, pixel_mean, pixel_std, size_divisibility=32, topk=100, thing_classes=None):
        super().__init__()
        self.net = net
        self.register_buffer("pixel_mean", torch.as_tensor(pixel_mean, dtype=torch.float32).view(1, -1, 1, 1), False)
        self.register_buffer("pixel_std", torch.as_tensor(pixel_std, dtype=torch.float32).view(1, -1, 1, 1), False)
        if self.pixel_mean.shape[1] != 3 or self.pixel_std.shape[1] != 3:
            raise L.MalError("InstanceSegmenter: pixel_mean and pixel_std hold three values (B, G, R)")
        self.size_divisibility = int(size_divisibility)
        self.topk = int(topk)
        self.thing_classes = thing_classes

    def preprocess(self, images):
        x = (images.flip(1) * 255.0 - self.pixel_mean.to(images.device)) / self.pixel_std.to(images.device)
        H, W = images.shape[2:]
        d = self.size_divisibility
        if d > 1:
            x = F.pad(x, (0, -W % d, 0, -H % d))
        return x

    @torch.no_grad()
    def forward(self, images):
        if not torch.is_tensor(images) or not images.is_cuda:
            raise L.MalError("InstanceSegmenter: images must be a device tensor (there is no CPU path)")
        if images.dim() != 4 or images.shape[1] != 3 or images.dtype != torch.float32:
            raise L.MalError("InstanceSegmenter: images must be (N,3,H,W) float32 RGB in [0, 1], got %s %s"
                             % (tuple(images.shape), images.dtype))
        out = self.net(self.preprocess(images))
        return instance_inference(out["pred_logits"], out["pred_masks"], images.shape[2:], self.topk, self.thing_classes)
