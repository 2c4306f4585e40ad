"""Multi-scale deformable attention, forward only, for the segmenter that feeds the temporal hint: the operator of
Mask2Former's pixel decoder (``mask2former/modeling/pixel_decoder/ops``).  Upstream ships it as a CUDA-only torch
extension, ``MultiScaleDeformableAttention``, which ``ops/functions/ms_deform_attn_func.py:21-29`` imports when the module
is imported; without it the reference's ``mask2former`` package does not import at all.  Here it is one HIP launch
(``mal_msda_fwd`` / ``mal_msda_fused_fwd``, include/mal_hip.h, mal_amd/csrc/mal_msda.hip).

Three ways in:

``ms_deform_attn(value, spatial_shapes, level_start_index, sampling_locations, attention_weights)``
    the operator itself, upstream's layouts, fp32 on the device.

``install_extension()``
    registers a module named ``MultiScaleDeformableAttention`` with upstream's two functions
    (``ops/src/vision.cpp:18-21``), so that the reference's unmodified ``mask2former`` package imports and its
    ``MSDeformAttnFunction.apply`` runs this kernel.  Call it before ``import mask2former``.

``MSDeformAttn``
    upstream's module (``ops/modules/ms_deform_attn.py``): same constructor, parameters, initialisation, ``forward``
    signature and ``state_dict``; Mask2Former checkpoints load.  With ``fused=True`` (the default) the softmax over the
    L*P logits and the location arithmetic (:104-112) happen inside the kernel.

Inference only.  The segmenter is frozen upstream (``ins_model.eval()``, manydepth/trainer.py:354) and called under
``torch.no_grad()`` (manydepth/dyn_utils.py:185-186), so no backward pass exists; asking for one raises
``NotImplementedError`` by name instead of returning a tensor without a graph.
"""
from __future__ import annotations

import ctypes
import math
import sys
import types
import warnings

import torch
from torch import nn

from . import _lib as L
from . import ops

EXTENSION_NAME = "MultiScaleDeformableAttention"
NO_BACKWARD = ("mal_amd.msda implements the forward pass of multi-scale deformable attention only: the segmenter is frozen "
               "(ins_model.eval(), manydepth/trainer.py:354) and is called under torch.no_grad() "
               "(manydepth/dyn_utils.py:185-186), so no gradient is ever taken through it")

_LEVELS = {}  # (shapes, starts, device) -> (spatial_shapes, level_start_index) on the device


def check_levels(spatial_shapes, level_start_index, S):
    """Host-side check of a level table given as lists or CPU tensors: L rows (H_l, W_l) >= 1, sum H_l W_l == S and
    level_start_index[l] == sum of the levels before l.  -> (tuple of (H, W), tuple of starts)."""
    hw = spatial_shapes.tolist() if torch.is_tensor(spatial_shapes) else [list(r) for r in spatial_shapes]
    st = level_start_index.tolist() if torch.is_tensor(level_start_index) else list(level_start_index)
    if not hw or any(len(r) != 2 for r in hw):
        raise L.MalError("ms_deform_attn: spatial_shapes must hold L >= 1 rows (H_l, W_l), got %r" % (hw,))
    hw = tuple((int(h), int(w)) for h, w in hw)
    st = tuple(int(s) for s in st)
    if len(st) != len(hw):
        raise L.MalError("ms_deform_attn: %d levels in spatial_shapes, %d entries in level_start_index" % (len(hw), len(st)))
    if any(h < 1 or w < 1 for h, w in hw):
        raise L.MalError("ms_deform_attn: every level must be at least 1x1, got %r" % (hw,))
    total = sum(h * w for h, w in hw)
    if total != int(S):
        raise L.MalError("ms_deform_attn: the levels %r hold %d positions, value holds S = %d" % (hw, total, int(S)))
    at = 0
    for l, (h, w) in enumerate(hw):
        if st[l] != at:
            raise L.MalError("ms_deform_attn: level_start_index[%d] is %d, the levels before it hold %d positions"
                             % (l, st[l], at))
        at += h * w
    return hw, st


def _levels(spatial_shapes, level_start_index, S, dev):
    """-> int64 device tensors (L,2) and (L).  Device tensors pass through unread (the kernel guards every level); host
    lists and CPU tensors are checked here and uploaded once per (table, device)."""
    on_dev = [torch.is_tensor(t) and t.is_cuda for t in (spatial_shapes, level_start_index)]
    if all(on_dev):
        if spatial_shapes.dim() != 2 or spatial_shapes.shape[1] != 2 or level_start_index.shape != spatial_shapes.shape[:1]:
            raise L.MalError("ms_deform_attn: spatial_shapes must be (L, 2) and level_start_index (L), got %s and %s"
                             % (tuple(spatial_shapes.shape), tuple(level_start_index.shape)))
        return (spatial_shapes.to(device=dev, dtype=torch.int64).contiguous(),
                level_start_index.to(device=dev, dtype=torch.int64).contiguous())
    if any(on_dev):  # one on the device, one on the host: bring the device one over (a readback the caller chose)
        spatial_shapes = spatial_shapes.cpu() if on_dev[0] else spatial_shapes
        level_start_index = level_start_index.cpu() if on_dev[1] else level_start_index
    hw, st = check_levels(spatial_shapes, level_start_index, S)
    key = (hw, st, str(dev))
    if key not in _LEVELS:
        _LEVELS[key] = (torch.tensor(hw, dtype=torch.int64).to(dev), torch.tensor(st, dtype=torch.int64).to(dev))
    return _LEVELS[key]


def _f32(t, name):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise L.MalError("ms_deform_attn: %s must be a device tensor (there is no CPU path)" % name)
    if t.dtype != torch.float32:
        raise L.MalError("ms_deform_attn: %s must be float32, got %s (fp16 / bf16 are not built)" % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _refuse_grad(*tensors):
    if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors):
        raise NotImplementedError(NO_BACKWARD + "; call it under torch.no_grad()")


def _launch(entry, value, spatial_shapes, level_start_index, loc, wgt, ref):
    """shared by the two routes: ``loc`` (N,Lq,M,L,P,2) locations or offsets, ``wgt`` (N,Lq,M,L,P) or (N,Lq,M,L*P)
    weights or logits, ``ref`` None or (N,Lq,L,2|4)"""
    _refuse_grad(value, loc, wgt, ref)
    value, loc, wgt = _f32(value, "value"), _f32(loc, "sampling_locations"), _f32(wgt, "attention_weights")
    if value.dim() != 4:
        raise L.MalError("ms_deform_attn: value must be (N, S, M, D), got %s" % (tuple(value.shape),))
    if loc.dim() != 6 or loc.shape[5] != 2:
        raise L.MalError("ms_deform_attn: sampling_locations must be (N, Lq, M, L, P, 2), got %s" % (tuple(loc.shape),))
    N, S, M, D = value.shape
    _, Lq, _, nl, P, _ = loc.shape
    if tuple(loc.shape[:3]) != (N, Lq, M):
        raise L.MalError("ms_deform_attn: sampling_locations is %s, value %s" % (tuple(loc.shape), tuple(value.shape)))
    if tuple(wgt.shape[:3]) != (N, Lq, M) or wgt.numel() != N * Lq * M * nl * P:
        raise L.MalError("ms_deform_attn: attention_weights is %s, expected (%d, %d, %d, %d, %d)"
                         % (tuple(wgt.shape), N, Lq, M, nl, P))
    dev = value.device
    if loc.device != dev or wgt.device != dev:
        raise L.MalError("ms_deform_attn: the inputs are on %s, %s and %s" % (dev, loc.device, wgt.device))
    shapes, start = _levels(spatial_shapes, level_start_index, S, dev)
    if shapes.shape[0] != nl:
        raise L.MalError("ms_deform_attn: %d levels in spatial_shapes, %d in sampling_locations" % (shapes.shape[0], nl))
    ref_dim = 0
    if ref is not None:
        ref = _f32(ref, "reference_points")
        if ref.dim() != 4 or tuple(ref.shape[:3]) != (N, Lq, nl) or ref.shape[3] not in (2, 4) or ref.device != dev:
            raise L.MalError("ms_deform_attn: reference_points must be (%d, %d, %d, 2 or 4) on %s, got %s on %s"
                             % (N, Lq, nl, dev, tuple(ref.shape), ref.device))
        ref_dim = ref.shape[3]
    lib, p = L.load(), ops._p
    with torch.cuda.device(dev):
        out = torch.empty((N, Lq, M * D), dtype=torch.float32, device=dev)
        a = L.MsdaArgs()
        a.value, a.spatial_shapes, a.level_start_index = p(value), p(shapes), p(start)
        a.sampling_locations, a.attention_weights, a.reference_points = p(loc), p(wgt), p(ref)
        a.N, a.S, a.M, a.D, a.L, a.P, a.Lq, a.ref_dim = N, S, M, D, nl, P, Lq, ref_dim
        a.out, a.stream = p(out), ops._stream()
        L.check(getattr(lib, entry)(ctypes.byref(a)), entry)
    return out


def plan(N, S, Lq, M, D, nl, P, aligned=True):
    """-> (channels a lane owns, rows (n, q, m) per workgroup, workgroups, dynamic LDS bytes) of either route's launch for
    that shape (``nl`` levels), with value and out that are (``aligned``) or are not on the 16-byte grid: ``mal_msda_plan``,
    pure host code, the function both entry points take their launch from.  A shape they refuse raises."""
    vec, rows, blocks, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    L.check(L.load().mal_msda_plan(int(N), int(S), int(Lq), int(M), int(D), int(nl), int(P), int(bool(aligned)),
                                   ctypes.byref(vec), ctypes.byref(rows), ctypes.byref(blocks), ctypes.byref(lds)),
            "mal_msda_plan")
    return vec.value, rows.value, blocks.value, lds.value


def ms_deform_attn(value, spatial_shapes, level_start_index, sampling_locations, attention_weights):
    """value (N,S,M,D), sampling_locations (N,Lq,M,L,P,2) in (x, y) order in [0,1] over the padded map,
    attention_weights (N,Lq,M,L,P), fp32 on the device -> (N, Lq, M*D).  ``spatial_shapes`` (L,2) rows (H_l, W_l) and
    ``level_start_index`` (L): int64 device tensors (read by the kernel, no synchronisation) or host lists / CPU tensors
    (checked on the host, uploaded once).  Strided inputs are copied."""
    return _launch("mal_msda_fwd", value, spatial_shapes, level_start_index, sampling_locations, attention_weights, None)


def ms_deform_attn_fused(value, spatial_shapes, level_start_index, sampling_offsets, attention_logits, reference_points):
    """The module's route in one launch: ``sampling_offsets`` (N,Lq,M,L,P,2) and ``attention_logits`` (N,Lq,M,L*P) are the
    raw outputs of the two linear layers, ``reference_points`` (N,Lq,L,2) or (N,Lq,L,4); the softmax over L*P and
    upstream's location arithmetic (ops/modules/ms_deform_attn.py:104-112) happen in the kernel."""
    return _launch("mal_msda_fused_fwd", value, spatial_shapes, level_start_index, sampling_offsets, attention_logits,
                   reference_points)


# ---- the extension's two functions, names and argument order of ops/src/vision.cpp:18-21 ---------------------------------
def ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step):
    """``im2col_step`` is upstream's batch chunk; one launch covers the batch here and the argument is ignored."""
    return ms_deform_attn(value, spatial_shapes, level_start_index, sampling_loc, attn_weight)


def ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, im2col_step):
    raise NotImplementedError(NO_BACKWARD)


def install_extension():
    """Register this module's forward and (refusing) backward as ``sys.modules["MultiScaleDeformableAttention"]``.
    Idempotent; a real extension that is already loaded is not replaced."""
    have = sys.modules.get(EXTENSION_NAME)
    if have is not None:
        if getattr(have, "__mal_amd__", False):
            return have
        raise L.MalError("a %s extension is already loaded (%s); mal_amd.msda.install_extension() does not replace it"
                         % (EXTENSION_NAME, getattr(have, "__file__", "no file")))
    mod = types.ModuleType(EXTENSION_NAME, "mal_amd.msda: multi-scale deformable attention in HIP, forward only")
    mod.ms_deform_attn_forward = ms_deform_attn_forward
    mod.ms_deform_attn_backward = ms_deform_attn_backward
    mod.__mal_amd__ = True
    sys.modules[EXTENSION_NAME] = mod
    return mod


class MSDeformAttn(nn.Module):
    """Upstream's module of the same name: four linear layers around the operator, parameters and ``state_dict`` keys as
    upstream's (``sampling_offsets``, ``attention_weights``, ``value_proj``, ``output_proj``).  ``fused``: the softmax and
    the sampling locations are formed inside the kernel (one launch instead of three ATen passes and one)."""

    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4, fused=True):
        super().__init__()
        if d_model % n_heads:
            raise ValueError("d_model must be divisible by n_heads, but got {} and {}".format(d_model, n_heads))
        d_head = d_model // n_heads
        if d_head & (d_head - 1):
            warnings.warn("MSDeformAttn: %d channels per head; a multiple of 4 takes the float4 path of the kernel" % d_head)
        self.im2col_step = 128  # upstream's attribute; not used by the kernel
        self.d_model, self.n_levels, self.n_heads, self.n_points = d_model, n_levels, n_heads, n_points
        self.fused = bool(fused)
        self.sampling_offsets = nn.Linear(d_model, n_heads * n_levels * n_points * 2)
        self.attention_weights = nn.Linear(d_model, n_heads * n_levels * n_points)
        self.value_proj = nn.Linear(d_model, d_model)
        self.output_proj = nn.Linear(d_model, d_model)
        self._reset_parameters()

    def _reset_parameters(self):
        """Upstream's initial state: zero offset and attention weights, offset biases that point head m in direction
        2 pi m / M (scaled to the unit square's border) with point i at i + 1 steps, Xavier projections."""
        M, nl, P = self.n_heads, self.n_levels, self.n_points
        with torch.no_grad():
            angle = torch.arange(M, dtype=torch.float32) * (2.0 * math.pi / M)
            step = torch.stack([angle.cos(), angle.sin()], -1)
            step = step / step.abs().max(-1, keepdim=True)[0]
            bias = step.view(M, 1, 1, 2) * torch.arange(1, P + 1, dtype=torch.float32).view(1, 1, P, 1)
            self.sampling_offsets.weight.zero_()
            self.sampling_offsets.bias.copy_(bias.expand(M, nl, P, 2).reshape(-1))
            self.attention_weights.weight.zero_()
            self.attention_weights.bias.zero_()
            for proj in (self.value_proj, self.output_proj):
                nn.init.xavier_uniform_(proj.weight)
                proj.bias.zero_()

    def forward(self, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index,
                input_padding_mask=None):
        """query (N,Lq,C), reference_points (N,Lq,L,2) or (N,Lq,L,4) in [0,1] over the padded maps, input_flatten
        (N,S,C), input_spatial_shapes (L,2), input_level_start_index (L), input_padding_mask (N,S) bool, True = padding
        -> (N,Lq,C)"""
        _refuse_grad(query, reference_points, input_flatten, *self.parameters())
        N, Lq, _ = query.shape
        S = input_flatten.shape[1]
        M, nl, P = self.n_heads, self.n_levels, self.n_points
        if reference_points.shape[-1] not in (2, 4):
            raise ValueError("Last dim of reference_points must be 2 or 4, but get {} instead.".format(reference_points.shape[-1]))
        if not input_flatten.is_cuda:
            raise L.MalError("MSDeformAttn: the inputs must be device tensors (there is no CPU path)")
        shapes, start = _levels(input_spatial_shapes, input_level_start_index, S, input_flatten.device)
        value = self.value_proj(input_flatten)
        if input_padding_mask is not None:
            value = value.masked_fill(input_padding_mask[..., None], 0.0)
        value = value.view(N, S, M, self.d_model // M)
        offsets = self.sampling_offsets(query).view(N, Lq, M, nl, P, 2)
        logits = self.attention_weights(query).view(N, Lq, M, nl * P)
        if self.fused:
            out = ms_deform_attn_fused(value, shapes, start, offsets, logits, reference_points)
        else:
            weights = torch.softmax(logits, -1).view(N, Lq, M, nl, P)
            if reference_points.shape[-1] == 2:
                wh = shapes.flip(-1)  # (W_l, H_l)
                locations = reference_points[:, :, None, :, None, :] + offsets / wh[None, None, None, :, None, :]
            else:
                locations = reference_points[:, :, None, :, None, :2] + offsets / P * reference_points[:, :, None, :, None, 2:] * 0.5
            out = ms_deform_attn(value, shapes, start, locations, weights)
        return self.output_proj(out)
