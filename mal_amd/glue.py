"""The glue between two convolutions of the depth decoder as one HIP pass each way (mal_amd/csrc/mal_glue.hip):

    F.pad(torch.cat([F.interpolate(F.elu(x), scale_factor=up, mode="nearest"), skip], 1), (1, 1, 1, 1), mode="reflect")

``decoder_join`` is what ``networks.DepthDecoder(fused_glue=True)`` calls at its 11 padding sites.  CUDA/HIP float32
tensors only; there is no CPU path -- a CPU tensor raises ``MalError``.

And the glue behind a ResNet convolution as two HIP launches each way (mal_amd/csrc/mal_bn.hip):

    F.relu(bn(x) + residual)                      bn an nn.BatchNorm2d, residual and the ReLU optional

``bn_join`` is what ``networks.BasicBlock`` and the encoders' stems call with ``fused_glue`` set (20 sites per ResNet-18).

And the max-pool behind the stem as one HIP launch each way (mal_amd/csrc/mal_pool.hip):

    F.max_pool2d(y, kernel_size=3, stride=2, padding=1)

``stem_pool`` is what the three encoders call with ``fused_pool`` set.
"""
from __future__ import annotations

import ctypes
import functools

import torch
import torch.nn.functional as F
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


@functools.lru_cache(maxsize=None)
def decoder_join_plan(B, C, Cs, h, w, up=2, need_x=True, need_skip=True):
    """-> (workgroups of mal_decoder_join_fwd, workgroups of mal_decoder_join_bwd for those outputs, floats of the flat
    output a workgroup covers per sweep) for that shape: pure host code.  A grid smaller than the output is strided over."""
    fwd, bwd, per = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    L.check(L.load().mal_decoder_join_plan(int(B), int(C), int(Cs), int(h), int(w), int(up), int(bool(need_x)),
                                           int(bool(need_skip)), ctypes.byref(fwd), ctypes.byref(bwd), ctypes.byref(per)),
            "mal_decoder_join_plan")
    return fwd.value, bwd.value, per.value


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


# ------------------------------------------------------------------ batch norm, residual add and ReLU behind a convolution
@functools.lru_cache(maxsize=None)
def bn_join_plan(B, C, H, W):
    """-> (blocks per channel, workspace bytes) of mal_bn_join_fwd / _bwd for that shape: pure host code"""
    blocks, nbytes = ctypes.c_int(0), ctypes.c_size_t(0)
    L.check(L.load().mal_bn_join_plan(int(B), int(C), int(H), int(W), ctypes.byref(blocks), ctypes.byref(nbytes)),
            "mal_bn_join_plan")
    return blocks.value, nbytes.value


_BN_WS = {}


def _bn_workspace(device, nbytes):
    """the partials of one direction live from its first launch to its second, both on the current stream: one buffer per
    (device, stream, size) serves every call, so the steady state allocates nothing"""
    key = (device.index, _stream(), nbytes)
    ws = _BN_WS.get(key)
    if ws is None:
        ws = _BN_WS[key] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
    return ws


def bn_join_fallback_reason(x, bn, residual=None):
    """why ``bn_join`` runs the module's own ATen composition for these arguments instead of the kernels, or None"""
    if x.dim() != 4:
        return "x is not (B,C,H,W)"
    if x.dtype != torch.float32:
        return "dtype other than float32"
    if not x.is_contiguous():
        return "x is not contiguous NCHW"
    if residual is not None and (residual.dtype != x.dtype or residual.shape != x.shape or residual.device != x.device
                                 or not residual.is_contiguous()):
        return "residual is not a contiguous float32 tensor of x's shape"
    if not bn.affine or bn.weight is None or bn.bias is None:
        return "affine=False"
    if not bn.track_running_stats or bn.running_mean is None or bn.running_var is None:
        return "track_running_stats=False"
    if bn.momentum is None:
        return "momentum=None (cumulative average)"
    if not bn.training and torch.is_grad_enabled() and any(
            t is not None and t.requires_grad for t in (x, residual, bn.weight, bn.bias)):
        return "eval mode with a gradient requested"
    if x.numel() >= 2 ** 31:
        return "2^31 elements or more"
    return None


def _bn_aten(x, bn, residual, relu):
    out = bn(x)
    if residual is not None:
        out = out + residual
    return F.relu(out) if relu else out


def bn_join_fwd(x, bn, residual=None, relu=True):
    """the two forward launches -> (y, save_mean, save_invstd); the saved statistics are (C) fp64, None in eval mode.  In training
    mode the module's running statistics and num_batches_tracked are updated on the device."""
    B, C, H, W = x.shape
    training = bool(bn.training)
    y = torch.empty_like(x)
    save_mean = save_invstd = ws = None
    nbytes = 0
    if training:
        save_mean, save_invstd = torch.empty((2, C), dtype=torch.float64, device=x.device)  # fp64 until their last use
        nbytes = bn_join_plan(B, C, H, W)[1]
        ws = _bn_workspace(x.device, nbytes)
    L.check(L.load().mal_bn_join_fwd(_p(x), _p(residual), _p(bn.weight), _p(bn.bias), _p(bn.running_mean), _p(bn.running_var),
                                     _p(bn.num_batches_tracked) if training else None, _p(y), _p(save_mean), _p(save_invstd),
                                     B, C, H, W, float(bn.eps), float(bn.momentum), int(training), int(bool(relu)), _p(ws),
                                     nbytes, _stream()), "mal_bn_join_fwd")
    return y, save_mean, save_invstd


def bn_join_bwd(g_out, x, y, weight, save_mean, save_invstd, relu=True, need_x=True, need_r=True, need_w=True, need_b=True):
    """the adjoint of the training-mode forward -> (dx, dr, dgamma, dbeta), None where not asked for.  ``y`` (the forward's
    output) is read only with ``relu``; without it dr is the cotangent itself."""
    g_out = _req(g_out, "g_out")
    B, C, H, W = x.shape
    dev = x.device
    dx = torch.empty_like(x) if need_x else None
    dr = None
    if need_r:
        dr = torch.empty_like(x) if relu else g_out
    dw = db = None
    if need_w and need_b:
        dw, db = torch.empty((2, C), dtype=torch.float32, device=dev)
    elif need_w or need_b:
        dw, db = (torch.empty(C, dtype=torch.float32, device=dev) if need else None for need in (need_w, need_b))
    ws, nbytes = None, 0
    if need_x or need_w or need_b:
        nbytes = bn_join_plan(B, C, H, W)[1]
        ws = _bn_workspace(dev, nbytes)
    if need_x or need_w or need_b or (need_r and relu):
        L.check(L.load().mal_bn_join_bwd(_p(g_out), _p(x), _p(y) if relu else None, _p(weight), _p(save_mean), _p(save_invstd),
                                         _p(dx), _p(dr) if relu else None, _p(dw), _p(db), B, C, H, W, int(bool(relu)), _p(ws),
                                         nbytes, _stream()), "mal_bn_join_bwd")
    return dx, dr, dw, db


class BnJoinFn(Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, bn, relu):
        y, save_mean, save_invstd = bn_join_fwd(x, bn, residual, relu)
        ctx.relu = bool(relu)
        if bn.training:  # the mask of the ReLU is read from y: autograd's version check refuses a later write in place
            ctx.save_for_backward(x, y if relu else None, weight, save_mean, save_invstd)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        x, y, weight, save_mean, save_invstd = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, dr, dw, db = bn_join_bwd(g_out, x, y, weight, save_mean, save_invstd, ctx.relu, need[0], need[1], need[2], need[3])
        return dx, dr, dw, db, None, None


def bn_join(x, bn, residual=None, relu=True):
    """``F.relu(bn(x) + residual)`` for an ``nn.BatchNorm2d`` module ``bn`` (``residual`` and ``relu`` optional), the
    module's running statistics and ``num_batches_tracked`` updated as the module does it -- also under ``no_grad``; once
    differentiable in training mode.  Where the kernels do not apply (``bn_join_fallback_reason``) the module's own ATen
    composition runs.  CPU tensors raise ``MalError``; one value per channel in training mode raises ``ValueError``."""
    if not x.is_cuda or (residual is not None and not residual.is_cuda):
        raise L.MalError("bn_join: expected CUDA/HIP tensors, got %s (mal_amd has no CPU fallback)"
                         % (x.device if not x.is_cuda else residual.device,))
    if bn_join_fallback_reason(x, bn, residual) is not None:
        return _bn_aten(x, bn, residual, relu)
    if bn.training and x.numel() // x.shape[1] == 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (x.size(),))
    return BnJoinFn.apply(x, residual, bn.weight, bn.bias, bn, relu)


# ------------------------------------------------------------------------------------ the 3x3 / 2 max-pool behind a stem
@functools.lru_cache(maxsize=None)
def stem_pool_plan(B, C, H, W, aligned=True):
    """-> (OH, OW, workgroups forward, workgroups backward, outputs a thread owns forward, elements of dy a thread owns
    backward) of mal_stem_pool_fwd / _bwd for that shape, with pointers that are (``aligned``) or are not on the 16-byte
    grid: pure host code.  A grid smaller than the tensor is strided over."""
    out = [ctypes.c_int(0) for _ in range(6)]
    L.check(L.load().mal_stem_pool_plan(int(B), int(C), int(H), int(W), int(bool(aligned)), *[ctypes.byref(o) for o in out]),
            "mal_stem_pool_plan")
    return tuple(o.value for o in out)


def _pool_shape(y):
    if y.dim() != 4:
        raise L.MalError("stem_pool: y must be (B,C,H,W), got %s" % (tuple(y.shape),))
    B, C, H, W = y.shape
    return B, C, H, W, (H - 1) // 2 + 1, (W - 1) // 2 + 1


def stem_pool_fwd(y, need_code=True):
    """-> (p, code): ``F.max_pool2d(y, 3, 2, 1)`` and, with ``need_code``, one byte per output: the winner's position kh*3 + kw
    in the unclipped window (None otherwise: nothing is allocated for it)"""
    y = _req(y, "y")
    B, C, H, W, OH, OW = _pool_shape(y)
    p = torch.empty((B, C, OH, OW), dtype=torch.float32, device=y.device)
    code = torch.empty((B, C, OH, OW), dtype=torch.uint8, device=y.device) if need_code else None
    L.check(L.load().mal_stem_pool_fwd(_p(y), _p(p), _p(code), B, C, H, W, _stream()), "mal_stem_pool_fwd")
    return p, code


def stem_pool_bwd(g_p, g_y, code, shape):
    """the adjoint, gathered in a fixed order: (cotangent of p, cotangent that reaches y from its other consumer, the forward's
    codes, y's shape) -> dy.  Either cotangent may be None; without ``g_p`` the result is ``g_y`` itself and nothing is launched."""
    if g_p is None:
        return g_y
    g_p, g_y = _req(g_p, "g_p"), _req(g_y, "g_y")
    B, C, H, W = shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if tuple(g_p.shape) != (B, C, OH, OW) or tuple(code.shape) != (B, C, OH, OW) or code.dtype != torch.uint8:
        raise L.MalError("stem_pool_bwd: g_p and code must be %s, got %s and %s" % ((B, C, OH, OW), tuple(g_p.shape), tuple(code.shape)))
    if g_y is not None and tuple(g_y.shape) != (B, C, H, W):
        raise L.MalError("stem_pool_bwd: g_y must be %s, got %s" % ((B, C, H, W), tuple(g_y.shape)))
    dy = torch.empty((B, C, H, W), dtype=torch.float32, device=g_p.device)
    L.check(L.load().mal_stem_pool_bwd(_p(g_p), _p(g_y), _p(code), _p(dy), B, C, H, W, _stream()), "mal_stem_pool_bwd")
    return dy


class StemPoolFn(Function):
    """y -> (y, p).  The input comes back as an output so that the cotangent of its other consumer (the decoder's skip) and the
    pool's arrive together in one backward, which writes their sum in one pass; the codes are all it saves."""

    @staticmethod
    def forward(ctx, y):
        ctx.set_materialize_grads(False)  # a missing cotangent arrives as None, not as a tensor of zeros
        ctx.shape = tuple(y.shape)
        p, code = stem_pool_fwd(y, need_code=True)
        ctx.save_for_backward(code)
        return y, p

    @staticmethod
    @once_differentiable
    def backward(ctx, g_y, g_p):
        (code,) = ctx.saved_tensors
        return stem_pool_bwd(g_p, g_y, code, ctx.shape)


def stem_pool_fallback_reason(y, pool=None):
    """why ``stem_pool`` runs the module's own ``nn.MaxPool2d`` for these arguments instead of the kernels, or None"""
    if pool is not None:
        if type(pool) is not torch.nn.MaxPool2d:
            return "not an nn.MaxPool2d"
        pair = torch.nn.modules.utils._pair
        for name, want in (("kernel_size", 3), ("stride", 2), ("padding", 1), ("dilation", 1)):
            if tuple(pair(getattr(pool, name))) != (want, want):
                return "%s other than %d" % (name, want)
        if pool.ceil_mode:
            return "ceil_mode=True"
        if pool.return_indices:
            return "return_indices=True"
    if y.dim() != 4:
        return "y is not (B,C,H,W)"
    if y.dtype != torch.float32:
        return "dtype other than float32"
    if not y.is_contiguous():
        return "y is not contiguous NCHW"
    if y.numel() >= 2 ** 31:
        return "2^31 elements or more"
    return None


def stem_pool(y, pool=None):
    """-> (y, p) with ``p = F.max_pool2d(y, kernel_size=3, stride=2, padding=1)`` (``pool``: the ``nn.MaxPool2d`` module this
    stands for).  Use the returned ``y`` wherever the stem feature goes besides the pool: with a gradient wanted it is an output
    of the same autograd node, so both cotangents are summed by the pool's one backward pass; once differentiable.  Under
    ``no_grad`` no codes are written.  Where the kernels do not apply (``stem_pool_fallback_reason``) the module's own call
    runs.  CPU tensors raise ``MalError``."""
    if not y.is_cuda:
        raise L.MalError("stem_pool: expected a CUDA/HIP tensor, got %s (mal_amd has no CPU fallback)" % (y.device,))
    if stem_pool_fallback_reason(y, pool) is not None:
        return y, (pool(y) if pool is not None else F.max_pool2d(y, kernel_size=3, stride=2, padding=1))
    if torch.is_grad_enabled() and y.requires_grad:
        return StemPoolFn.apply(y)
    return y, stem_pool_fwd(y, need_code=False)[0]
