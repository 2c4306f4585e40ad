"""The glue between two convolutions of the depth decoder as one HIP pass each way (mal_amd/csrc/mal_glue.hip):

    F.pad(torch.cat([F.interpolate(F.elu(x), scale_factor=up, mode="nearest"), skip], 1), (1, 1, 1, 1), mode="reflect")

``decoder_join`` is what ``networks.DepthDecoder(fused_glue=True)`` calls at its 11 padding sites.  CUDA/HIP float32
tensors only; there is no CPU path -- a CPU tensor raises ``MalError``.
"""
from __future__ import annotations

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib as L
from .ops import _p, _req, _stream


def _dims(x, skip, up):
    if x.dim() != 4:
        raise L.MalError("decoder_join: x must be (B,C,h,w), got %s" % (tuple(x.shape),))
    B, C, h, w = x.shape
    Cs = 0
    if skip is not None:
        if skip.dim() != 4 or skip.shape[0] != B or tuple(skip.shape[2:]) != (up * h, up * w):
            raise L.MalError("decoder_join: skip must be (%d,Cs,%d,%d), got %s" % (B, up * h, up * w, tuple(skip.shape)))
        if skip.device != x.device:
            raise L.MalError("decoder_join: x is on %s, skip on %s" % (x.device, skip.device))
        Cs = skip.shape[1]
    return B, C, Cs, h, w


def decoder_join_fwd(x, skip=None, up=2, elu=True):
    """-> (B, C+Cs, up*h+2, up*w+2): activation, nearest upsampling, concatenation and reflection padding in one launch"""
    x, skip = _req(x, "x"), _req(skip, "skip")
    B, C, Cs, h, w = _dims(x, skip, up)
    out = torch.empty((B, C + Cs, up * h + 2, up * w + 2), dtype=torch.float32, device=x.device)
    L.check(L.load().mal_decoder_join_fwd(_p(x), _p(skip) if Cs else None, _p(out), B, C, Cs, h, w, int(up), int(bool(elu)),
                                          _stream()), "mal_decoder_join_fwd")
    return out


def decoder_join_bwd(g_out, x, Cs, up=2, elu=True, need_x=True, need_skip=True, shape=None):
    """the adjoint, gathered in a fixed order: cotangent of the padded tensor -> (gx or None, gskip or None).  ``x`` is
    read only with ``elu`` (it may be None otherwise; ``shape`` = (B,C,h,w) then says what it was)."""
    g_out = _req(g_out, "g_out")
    x = _req(x, "x") if elu else None
    B, C, h, w = x.shape if x is not None else shape
    if tuple(g_out.shape) != (B, C + Cs, up * h + 2, up * w + 2):
        raise L.MalError("decoder_join_bwd: g_out must be %s, got %s" % ((B, C + Cs, up * h + 2, up * w + 2), tuple(g_out.shape)))
    need_skip = need_skip and Cs > 0
    gx = torch.empty((B, C, h, w), dtype=torch.float32, device=g_out.device) if need_x else None
    gskip = torch.empty((B, Cs, up * h, up * w), dtype=torch.float32, device=g_out.device) if need_skip else None
    if need_x or need_skip:
        L.check(L.load().mal_decoder_join_bwd(_p(g_out), _p(x), _p(gx), _p(gskip), B, C, Cs, h, w, int(up), int(bool(elu)),
                                              _stream()), "mal_decoder_join_bwd")
    return gx, gskip


class DecoderJoinFn(Function):
    @staticmethod
    def forward(ctx, x, skip, up, elu):
        ctx.cfg = (int(up), bool(elu), tuple(x.shape), 0 if skip is None else skip.shape[1])
        out = decoder_join_fwd(x, skip, up, elu)
        if elu:  # the derivative of the activation is the only thing the adjoint reads of the inputs
            ctx.save_for_backward(x)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        up, elu, shape, Cs = ctx.cfg
        x = ctx.saved_tensors[0] if elu else None
        need_skip = Cs > 0 and ctx.needs_input_grad[1]
        gx, gskip = decoder_join_bwd(g_out, x, Cs, up, elu, ctx.needs_input_grad[0], need_skip, shape)
        return gx, gskip, None, None


def decoder_join(x, skip=None, up=2, elu=True):
    """``F.pad(cat([interpolate(F.elu(x), scale_factor=up, mode="nearest"), skip], 1), (1,1,1,1), mode="reflect")`` with
    ``up`` in {1, 2}, the activation optional (``elu=False``) and ``skip`` optional; once differentiable."""
    if up not in (1, 2):
        raise L.MalError("decoder_join: up must be 1 or 2, got %r" % (up,))
    return DecoderJoinFn.apply(x, skip, up, elu)
