"""The whole loss half of ``Trainer.process_batch`` (manydepth/trainer.py:573-642, ``--distil``)
as one C call forward (``mal_loss_step_fwd``, 5 kernels) and one backward
(``mal_loss_step_bwd``, 2 kernels): no Python between the kernels, no per-op autograd nodes.

``loss_step(...)`` returns the same ``losses`` dict keys as the reference's ``process_batch``
(views of one 16-float device vector, so reading them launches nothing) plus the per-pixel maps.
The operator-level API (``mal_amd.loss_utils`` / ``MALLossPath``) computes the same thing op by
op; ``tests/test_gpu_step.py`` holds the two against each other and against the CPU checker.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import inspect
from collections import namedtuple
from typing import Any, NamedTuple

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib as L
from . import config, loss_utils, ops

POISON_COTANGENTS = False  # tests: the cotangent buffers of a hinted step's synthesised pair start as NaN instead of uninitialised
_NOISE_COUNTER = {}  # per device: the step number of the "philox" noise stream, a device word the step itself advances


# The records the autograd functions take as ``consts`` / ``cfg``.  They ARE tuples in the positional order the functions
# have always read (a plain tuple of any length accepted before still is: forward() normalises with ``StepCfg(*cfg)``).
class StepConsts(NamedTuple):
    color0: Any; color_m1: Any; color_p1: Any; K: Any; inv_K: Any
    cmask: Any; keep: Any  # outputs["consistency_mask"]; (B,) 1 - augmentation_mask, or the mask itself (cfg.aug_is_mask)
    lowest: Any; noise: Any  # outputs["lowest_cost"]; (B,1,H,W) N(0,1), None with cfg.philox


class StepCfg(NamedTuple):
    min_depth: float; max_depth: float; no_ens: bool; w_main: float; w_distil: float; want_maps: bool; aug_is_mask: bool
    want_decisions: bool  # parity instrumentation (tests): the kernels' per-pixel decisions, MAL_DEC_* planes
    philox: Any           # None, or (seed, want the drawn values back)
    dual_distil: bool = False


class MsConsts(NamedTuple):
    colors: Any; colors_s: Any  # (color0, color_m1, color_p1); inputs[("color", 0, s)] for s = 1..sclm
    K: Any; inv_K: Any; cmask: Any; keep: Any
    lowest: Any; noises: Any  # nullable: no matching mask; one (B,1,H,W) map per scale, or None


class MsCfg(NamedTuple):
    min_depth: float; max_depth: float; sclm: int; aug_is_mask: bool
    philox: Any; want_maps: bool  # None, or the seed
    hint: Any = None; no_ssim: bool = False  # --temporal: (image_synthesis, inputs, mono_outputs)
    extra_flags: int = 0          # MAL_STEP_NO_MOTION_MASK | MAL_STEP_NO_AUG | MAL_STEP_ENSEMBLE
    want_decisions: bool = False  # parity instrumentation (tests): per-scale decision planes


Kept = namedtuple("Kept", "tens cons ws losses total")  # ctx.keep: the C struct holds raw pointers, these keep the tensors alive


class V16:
    """slots of the 16-float loss vector of mal_loss_step_fwd (include/mal_hip.h:244-246)"""
    REPROJ_T, SMOOTH_T, LOSS_T, REPROJ_S, CONSISTENCY, SMOOTH_S, DISTIL, LOSS_MAIN, TOTAL, REPROJ_BOTH, LOSS_PLAIN, LOSS_BLC = range(12)


class V48:
    """slots of the 48-float loss vector of mal_loss_multiscale_fwd (include/mal_hip.h:448-451): ``at(net, scale, term)`` with
    net 0 the teacher, then the totals and the per-scale sums"""
    REPROJ, CONSISTENCY, SMOOTH, LOSS = range(4)
    TEACHER, STUDENT = 0, 1
    TEACHER_TOTAL, STUDENT_TOTAL, TOTAL = 32, 33, 34
    REPROJ_BOTH, LOSS_BOTH, ENSEMBLE = 36, 40, 44  # + scale
    at = staticmethod(lambda net, s, term: (net * L.MS_MAX_SCALES + s) * 4 + term)


def noise_counter(dev):
    """(1,) int64 device tensor: how many steps of the in-kernel ("philox") tie-break noise stream have been drawn"""
    t = _NOISE_COUNTER.get(dev.index)
    if t is None:
        t = _NOISE_COUNTER[dev.index] = torch.zeros(1, dtype=torch.int64, device=dev)
    return t


_WS_SLOT = 0


@contextlib.contextmanager
def workspace_slot(slot):
    """``with workspace_slot(k): loss_step(...)``: the steps issued inside keep their intermediate maps in workspace number
    ``k`` of this (device, stream, shape) instead of the shared one -- k steps in flight on ONE stream then do not overwrite
    each other's maps (a trainer that runs the backward of a step before the next forward never needs it; bench.py rotates
    over several batches with it, so that no step finds the previous replay's working set in the Infinity Cache)."""
    global _WS_SLOT
    prev, _WS_SLOT = _WS_SLOT, int(slot)
    try:
        yield
    finally:
        _WS_SLOT = prev


_BUFFERS = {}  # every cached device buffer of the one-call steps, by (kind, device index, stream, workspace slot, *rest)


def _cached(kind, dev, rest, make, fits=lambda buf: True):
    """the buffer of this kind on this device, stream and workspace slot: made on first use, again only when it no longer
    ``fits`` (rotating batches keep their own, a graph replay finds the captured ones)"""
    key = (kind, dev.index, ops._stream(), _WS_SLOT, *rest)
    buf = _BUFFERS.get(key)
    if buf is None or not fits(buf):
        buf = _BUFFERS[key] = make()
    return buf


def byte_workspace(kind, dev, need, *rest):
    """grow-only device byte workspace of a step family (``kind``) and shape (``rest``)"""
    return _cached(kind, dev, rest, lambda: torch.empty(need, dtype=torch.uint8, device=dev), lambda ws: ws.numel() >= need)


def _workspace(dev, B, H, W):
    return byte_workspace("step", dev, L.load().mal_step_workspace_bytes(B, H, W), B, H, W)


def map_names(cfg):
    """the per-pixel maps a single-scale step with this StepCfg returns, in output order"""
    names = ["mono_reproj", "multi_reproj", "consistency_mask"] + ([] if cfg.no_ens else ["ens_reproj"]) if cfg.want_maps else []
    names += ["noise"] if cfg.philox is not None and cfg.philox[1] else []
    return names + (["dec_teacher", "dec_student"] if cfg.want_decisions else [])


def _build_args(disp_t, disp_s, aa_m1, tr_m1, aa_p1, tr_p1, consts, cfg, temporal=False, ens_disp=None, main_temporal=False):
    """the mal_step_args block of one step, the tensors it points to (kept alive by the caller) and the map dict;
    ``ens_disp`` (--learn_ens): a seventh leaf, appended to the kept tensors"""
    color0, color_m1, color_p1, K, inv_K, cmask, keep, lowest, noise = consts
    no_ens, aug_is_mask, philox = cfg.no_ens, cfg.aug_is_mask, cfg.philox
    req = ops._req
    tens = [req(t, n) for t, n in ((disp_t, "disp_teacher"), (disp_s, "disp_student"), (aa_m1, "axisangle"),
                                   (tr_m1, "translation"), (aa_p1, "axisangle"), (tr_p1, "translation"))]
    if ens_disp is not None:
        tens.append(req(ens_disp, "ens_disp"))
        if tuple(tens[6].shape) != tuple(tens[0].shape):
            raise L.MalError("loss_step: outputs['ens_disp'] must have the shape of the disparities")
    # Zero-copy texels: three (B,3,H,W) images in torch.channels_last memory format ARE the (B,H,W,3) texel images the passes
    # gather from -- the step then skips the re-layout of its first sweep (MAL_STEP_TEXEL_INPUTS; same results bit for bit).
    # A loader gets there with `.contiguous(memory_format=torch.channels_last)` on the host tensor.
    texel_inputs = all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] == 3 and not t.is_contiguous()
                       and t.is_contiguous(memory_format=torch.channels_last) for t in (color0, color_m1, color_p1))
    cons = [t if texel_inputs else req(t, "input") for t in (color0, color_m1, color_p1)]
    cons += [req(t, "input") for t in (K, inv_K, cmask, keep, lowest)]
    cons.append(None if noise is None else req(noise, "input"))
    B, _, H, W = tens[0].shape
    dev = tens[0].device
    a = L.StepArgs()
    a.B, a.H, a.W = B, H, W
    a.min_depth, a.max_depth = float(cfg.min_depth), float(cfg.max_depth)
    a.flags = (L.STEP_NO_ENS if no_ens else 0) | (L.STEP_AUG_MASK if aug_is_mask else 0) | (L.STEP_TEMPORAL if temporal else 0) | \
              (L.STEP_DUAL_DISTIL if (cfg.dual_distil and no_ens) else 0) | (L.STEP_MAIN_TEMPORAL if main_temporal else 0) | \
              (L.STEP_TEXEL_INPUTS if texel_inputs else 0)  # (upstream reads dual_distil on the two-way branch only)
    if philox is not None:  # (seed, want the drawn values back)
        a.flags |= L.STEP_NOISE_PHILOX
        a.noise_seed = int(philox[0]) & 0xFFFFFFFFFFFFFFFF
        ctr = noise_counter(tens[0].device)
        a.noise_counter = ctr.data_ptr()
    a.w_main, a.w_distil = float(cfg.w_main), float(cfg.w_distil)
    p = ops._p
    a.disp_teacher, a.disp_student = p(tens[0]), p(tens[1])
    a.axisangle_m1, a.translation_m1, a.axisangle_p1, a.translation_p1 = (p(t) for t in tens[2:6])
    if ens_disp is not None:
        a.ens_disp = p(tens[6])
    (a.color0, a.color_m1, a.color_p1, a.K, a.inv_K, a.consistency_mask, a.augmentation_keep, a.lowest_cost,
     a.noise) = (p(t) for t in cons)
    losses = torch.empty(16, dtype=torch.float32, device=dev)
    total = torch.empty(1, dtype=torch.float32, device=dev)  # its own tensor: no select/copy nodes in the backward
    a.losses, a.loss_total = p(losses), p(total)
    maps = {}
    for k in map_names(cfg):
        if k.startswith("dec_"):  # the kernels' per-pixel decisions, MAL_DEC_* planes
            maps[k] = torch.zeros((L.DEC_PLANES, B, H, W), dtype=torch.int32, device=dev)
        else:
            maps[k] = torch.empty((B, H, W) if k == "consistency_mask" else (B, 1, H, W), dtype=torch.float32, device=dev)
    (a.mono_reproj, a.multi_reproj, a.consistency_mask_out, a.ens_reproj, a.noise_out, a.dec_teacher, a.dec_student) = (
        p(maps.get(k)) for k in ("mono_reproj", "multi_reproj", "consistency_mask", "ens_reproj", "noise", "dec_teacher", "dec_student"))
    ws = _workspace(dev, B, H, W)
    a.ws, a.ws_bytes, a.stream = p(ws), ws.numel(), ops._stream()
    return a, Kept(tens, cons, ws, losses, total), maps


def _input_positions(fn):
    """(inputs of the autograd function, position of ``ens_disp``): needs_input_grad and backward's result follow the signature"""
    names = list(inspect.signature(fn.forward).parameters)[1:]  # (without ctx)
    return len(names), names.index("ens_disp")


def _run_bwd(ctx, g_total, fn):
    """backward of ``fn`` (LossStepFn / TemporalLossStepFn): gradients for the six leaves and, at its position, ens_disp"""
    n_inputs, ens_index = fn.INPUTS
    tens = ctx.keep.tens
    ops.check_workspace(ctx.keep.ws, ctx.ws_token, "loss_step backward")
    # only the total is differentiable through this node: the 16 slots are its terms, for logging
    g_total = g_total.reshape(1).contiguous()
    a = ctx.args
    grads = [torch.empty_like(t) if ctx.needs_input_grad[i] else None for i, t in enumerate(tens[:6])]
    a.g_total = ops._p(g_total)
    (a.g_disp_teacher, a.g_disp_student, a.g_axisangle_m1, a.g_translation_m1, a.g_axisangle_p1,
     a.g_translation_p1) = (ops._p(g) for g in grads)
    g_ens = None
    if len(tens) > 6 and ctx.needs_input_grad[ens_index]:  # --learn_ens: the ensemble head's disparity
        g_ens = torch.empty_like(tens[6])
        a.g_ens_disp = ops._p(g_ens)
    L.check(L.load().mal_loss_step_bwd(C.byref(a)), "mal_loss_step_bwd")
    out = grads + [None] * (n_inputs - len(grads))
    out[ens_index] = g_ens
    return tuple(out)


def _end_fwd(ctx, a, keep, maps):
    """what both single-scale forwards leave for the backward, and their outputs: total, the 16 slots, the maps"""
    ctx.args, ctx.keep = a, keep  # the C struct holds raw pointers: keep the tensors alive
    ctx.ws_token = ops.claim_workspace(keep.ws)
    ctx.set_materialize_grads(False)
    outs = (keep.total, keep.losses, *maps.values())  # (the maps in map_names(cfg) order)
    ctx.mark_non_differentiable(*outs[1:])
    return outs


class LossStepFn(Function):
    """leaves: disp_teacher, disp_student, axisangle_m1, translation_m1, axisangle_p1, translation_p1."""

    @staticmethod
    def forward(ctx, disp_t, disp_s, aa_m1, tr_m1, aa_p1, tr_p1, consts, cfg, ens_disp=None):
        consts, cfg = StepConsts(*consts), StepCfg(*cfg)
        a, keep, maps = _build_args(disp_t, disp_s, aa_m1, tr_m1, aa_p1, tr_p1, consts, cfg, ens_disp=ens_disp)
        L.check(L.load().mal_loss_step_fwd(C.byref(a)), "mal_loss_step_fwd")
        if _CAPTURE is not None:
            _CAPTURE.append((a, keep))
        return _end_fwd(ctx, a, keep, maps)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_total, *_):
        if g_total is None:
            return (None,) * LossStepFn.INPUTS[0]
        return _run_bwd(ctx, g_total, LossStepFn)


LossStepFn.INPUTS = _input_positions(LossStepFn)


class _HintIO:
    """What ``_Hint`` and ``_ScaleHint`` share: the buffers of one (pass, scale) the producer is called on, their pointers in
    the argument block, the producer call and what is exposed of its answer."""

    def __init__(self, a, student, scale, pair, pre):
        """``a``: the argument block; ``scale``: index into its per-scale arrays, None where its members are plain pointers"""
        self.a, self.tag, self.student, self.scale = a, "_s" if student else "", student, scale
        # the two warped images of a sample side by side: the (2,3,H,W) pair the instance segmenter is fed is then a VIEW
        # (upstream stacks it per sample, dyn_utils.py:139-140); ("color", f, scale) are the two batch-strided halves
        self.pair = pair
        self.warp = [pair[:, 0], pair[:, 1]]
        self._set("warp", self.warp)
        # The buffers the synthesised images are made in are NOT filled: a producer that knows the key
        # ("syn_sparse_buffers", scale) -- mal_amd.dyn_utils.image_synthesis -- writes only the pixels of its instances'
        # regions into them instead of cloning every sample first (dyn_utils.py:127-128) and says so (("syn_sparse", scale),
        # with the region map); the sweep then reads the warped images everywhere else (MAL_STEP_SYN_SPARSE), so the pass in
        # front of the producer writes them once, not twice
        self.pre = pre
        self.has_ins, self.local = False, None

    def _put(self, name, ptr):
        if self.scale is None:
            setattr(self.a, name, ptr)
        else:
            getattr(self.a, name)[self.scale] = ptr

    def _set(self, base, tensors, tail=("_m1", "_p1")):
        for t, sfx in zip(tensors, tail):
            self._put(base + self.tag + sfx, t.data_ptr())

    def _call(self, synth, inputs, colors):
        """the producer on this scale's warped images (``colors``: the tensors it finds them under)"""
        sc = self.scale or 0
        local = {("color", -1, sc): colors[0], ("color", 1, sc): colors[1], ("color_pair", sc): self.pair,
                 ("syn_sparse_buffers", sc): (self.pre[0], self.pre[1])}
        self.has_ins = bool(synth(inputs, local, sc))
        self.local = local

    def _expose(self, out, dense, syn, region):
        """what the reference's generate_images_pred leaves in the pass's outputs dict (trainer.py:1122-1125,1161-1165):
        ("color", f, scale) and, with ``syn`` (None: the producer wrote none), ("syn", f, scale); ``region``: a sparse
        producer's map, None for a dense one"""
        sc = self.scale or 0
        out[("color", -1, sc)], out[("color", 1, sc)] = self.warp
        if syn is not None and region is None:
            out[("syn", -1, sc)], out[("syn", 1, sc)] = syn
        elif syn is not None and dense:
            # dense images for the caller (logging) only when maps are wanted: outside the regions syn IS the warped image
            inside = (region & 1).bool().unsqueeze(1)
            out[("syn", -1, sc)], out[("syn", 1, sc)] = (torch.where(inside, t, w_) for t, w_ in zip(syn, self.warp))


class _Hint(_HintIO):
    """One pass's exchange with the temporal hint's producer: the teacher's (``--temporal``, mal_step_args.warp_* / syn_* /
    g_syn_* / g_warp_* / syn_region) or the student's (``--main_temporal``, the ``*_s_*`` members)."""

    def __init__(self, a, student, B, H, W, dev, scale=None):
        """``scale`` (mal_ms_args, one hint per scale): the members are arrays indexed by it and the sparse bit lives in
        ``syn_sparse``; None: mal_step_args"""
        new = lambda shape: torch.empty(shape, dtype=torch.float32, device=dev)
        super().__init__(a, student, scale, new((B, 2, 3, H, W)), [new((B, 3, H, W)) for _ in range(2)])
        self.sparse_flag = L.STEP_SYN_S_SPARSE if student else L.STEP_SYN_SPARSE
        self.sparse, self.gsyn_sparse = False, False
        self.shape, self.dev = (B, 3, H, W), dev
        self.region, self.snap, self.syn, self.syn_data, self.leaf, self.g_syn = None, None, None, None, None, None

    def _mark_sparse(self):
        self.sparse = True
        if self.scale is None:
            self.a.flags |= self.sparse_flag
        else:
            self.a.syn_sparse |= 1 << self.scale

    def produce(self, synth, inputs, defer=False):
        """between mal_loss_step_warp and mal_loss_step_fwd; anything raised here is the caller's to abort the step on.
        ``defer``: the caller calls ``finish`` itself (with the has_ins every scale is to use)"""
        with torch.enable_grad():
            self.leaf = [w.detach().requires_grad_(True) for w in self.warp]
            self._call(synth, inputs, self.leaf)
        if not defer:
            self.finish()

    def finish(self, has_ins=None):
        """what the producer left -> the argument block (``has_ins``: overrides the producer's own answer -- the multi-scale
        path keeps the LAST scale's for all of them, trainer.py:1162)"""
        B, _, H, W = self.shape
        sc, local = self.scale or 0, self.local
        if has_ins is not None:
            if has_ins and not self.has_ins:
                raise KeyError(("syn", -1, sc))  # as upstream: compute_losses reads a key this scale's producer call never wrote
            self.has_ins = bool(has_ins)
        if self.has_ins:
            self.syn = [local[("syn", -1, sc)], local[("syn", 1, sc)]]
            self.syn_data = [ops._req(t.detach(), "syn") for t in self.syn]
            region = local.get(("syn_region", sc))
            sparse = bool(local.get(("syn_sparse", sc)))
            if sparse and (region is None or any(t.data_ptr() != q.data_ptr() for t, q in zip(self.syn_data, self.pre))):
                raise L.MalError("loss_step: ('syn_sparse', %d) needs the region map and the buffers of ('syn_sparse_buffers', %d)" % (sc, sc))
            if region is not None and not (region.is_cuda and region.dtype == torch.uint8 and tuple(region.shape) == (B, H, W)
                                           and region.is_contiguous()):
                raise L.MalError("loss_step: ('syn_region', %d) must be a contiguous (B,H,W) uint8 device tensor" % sc)
            self.region = region
            if region is not None:
                self._put("syn" + self.tag + "_region", region.data_ptr())
                if sparse:
                    self._mark_sparse()
                # ... and with the map the sweep leaves a second copy of d/d syn at the touched pixels: what the
                # producer's in-place backward gathers from
                self.snap = [torch.empty(self.shape, dtype=torch.float32, device=self.dev) for _ in range(2)]
                self._set("g_syn", self.snap, ("_region_m1", "_region_p1"))
        else:
            # no matched instance anywhere (loss_utils.py:84,152: only the two warped candidates enter the min): an all-zero
            # region map over the untouched buffers -- no synthesised candidate is evaluated anywhere (no pixel of them is
            # read), the running min passes through and d/d syn is zero
            self.syn, self.syn_data = None, self.pre
            self.region = torch.zeros((B, H, W), dtype=torch.uint8, device=self.dev)
            self._put("syn" + self.tag + "_region", self.region.data_ptr())
            self._mark_sparse()
        # the cotangents of syn: this node's own buffers, which the producer's backward may turn into its result in place
        self.g_syn = [torch.empty(self.shape, dtype=torch.float32, device=self.dev) for _ in range(2)]
        if POISON_COTANGENTS:
            for g in self.g_syn:
                g.fill_(float("nan"))
        self._set("syn", self.syn_data)
        self._set("g_syn", self.g_syn)
        self.gsyn_sparse = self._cotangent_never_read_densely()
        if self.gsyn_sparse:
            self.a.flags |= L.STEP_GSYN_SPARSE

    def _cotangent_never_read_densely(self):
        """MAL_STEP_GSYN_SPARSE: may the fused sweep leave the tiles of g_syn away from the region unwritten?  Only when the
        one reader besides the library's own gradient sweep provably touches region pixels alone: the teacher's pair at scale
        0, a sparse producer with its region map (or no instance at all: the identity, nothing reads g_syn), both syn tensors
        the outputs of ONE ``BatchSynthesisFn`` node whose image inputs are this hint's leaves themselves -- an autograd op
        in between would be handed the cotangent as a whole -- and the snapshots its region-only backward gathers from."""
        if not config.syn_grad_sparse or self.student or self.scale is not None or not self.sparse:
            return False
        if self.syn is None:
            return True
        return self.snap is not None and self._producer_on_leaves()

    def _producer_on_leaves(self):
        """both syn tensors are outputs of ONE ``BatchSynthesisFn`` node whose image inputs are this hint's leaves, nothing in
        between: the producer's backward is then the only operation ``torch.autograd.grad`` runs"""
        from . import dyn_utils
        fn = self.syn[0].grad_fn
        if fn is None or fn is not self.syn[1].grad_fn or not isinstance(fn, dyn_utils.BatchSynthesisFn._backward_cls):
            return False
        nxt = fn.next_functions
        return len(nxt) >= 2 and all(nxt[i][0] is not None and getattr(nxt[i][0], "variable", None) is self.leaf[i]
                                     for i in range(2))

    def expose(self, out, dense):
        self._expose(out, dense, self.syn_data if self.has_ins else None, self.region if self.sparse else None)
        out["multi_has_ins" if self.student else "has_ins"] = self.has_ins

    def backward(self, stream=None):
        """the producer's own backward (linear): g_syn -> g_warp, handed to mal_loss_step_bwd.  ``stream`` (option
        "tail_overlap"): a raw stream handle that already waits for the cotangents' producer; a producer whose backward is
        ONE launch on buffers it was handed (mal_amd.dyn_utils, in place, region-only) enqueues it there.  Returns whether
        everything this call enqueued went to that stream (the caller cancels the overlap otherwise)."""
        on_stream = False
        if self.syn is None:
            g_warp = self.g_syn  # the identity producer
            on_stream = stream is not None  # (nothing was enqueued at all)
        else:
            from . import dyn_utils
            # mal_amd.dyn_utils.image_synthesis turns the cotangent buffers into its result in place
            reg = {g.data_ptr(): (self.snap[i] if self.snap is not None else None) for i, g in enumerate(self.g_syn)}
            dyn_utils.INPLACE_COTANGENTS.update(reg)
            # (the side stream only when that backward is ALL that runs: an autograd op behind it -- a producer that wraps
            # image_synthesis -- runs on the caller's stream and would read the cotangents while the side stream still writes them)
            dyn_utils.BACKWARD_STREAM["handle"] = stream if self._producer_on_leaves() else None
            dyn_utils.BACKWARD_STREAM["used"] = False
            try:
                g_warp = torch.autograd.grad(self.syn, self.leaf, self.g_syn, allow_unused=True)
            finally:
                for k in reg:
                    dyn_utils.INPLACE_COTANGENTS.pop(k, None)
                used = dyn_utils.BACKWARD_STREAM["used"]
                dyn_utils.BACKWARD_STREAM["handle"], dyn_utils.BACKWARD_STREAM["used"] = None, False
            # ... and only if the result IS those buffers (no further operation of the autograd engine on the caller's stream)
            in_place = all(g is not None and g.data_ptr() == q.data_ptr() and g.is_contiguous() for g, q in zip(g_warp, self.g_syn))
            if self.gsyn_sparse and not in_place:
                # the forward left the tiles of g_syn away from the region unwritten (MAL_STEP_GSYN_SPARSE): a backward that
                # did not turn those very buffers into its result, region pixels only, has read memory nobody wrote
                raise L.MalError("loss_step backward: the producer's backward did not take its in-place, region-only form, but "
                                 "the step kept the cotangent of the synthesised pair sparse (config.syn_grad_sparse)")
            on_stream = bool(used) and in_place
            g_warp = [torch.zeros_like(w) if g is None else g.contiguous() for g, w in zip(g_warp, self.warp)]
        self.g_warp = g_warp
        self._set("g_warp", g_warp)
        return on_stream


def _scale_buffers(dev, B, H, W, student, s):
    """the (B,2,3,H,W) warped pair and the two syn buffers of scale ``s`` > 0 of a pass, cached like the workspaces"""
    new = lambda shape: torch.empty(shape, dtype=torch.float32, device=dev)
    return _cached("scale_hint", dev, (B, H, W, student, s), lambda: (new((B, 2, 3, H, W)), new((B, 3, H, W)), new((B, 3, H, W))))


class _ScaleHint(_HintIO):
    """Scale ``s`` > 0 of a hinted pass with --distil (mal_step_scales_args): generate_images_pred warps the full-resolution
    sources with ("disp", s) upsampled and calls the producer on them (trainer.py:1088-1165), but no loss reads what it
    leaves -- only its answer counts, and only the last scale's.  Forward only: the warped images carry no gradient and no
    backward is ever run for them."""

    def __init__(self, sa, student, s, B, H, W, dev):
        pair, pre0, pre1 = _scale_buffers(dev, B, H, W, student, s)
        super().__init__(sa, student, s, pair, (pre0, pre1))

    def produce(self, synth, inputs):
        with torch.no_grad():
            self._call(synth, inputs, self.warp)

    def expose(self, out, dense):
        """("color", f, s) and, where the producer wrote them, ("syn", f, s), as _Hint.expose does for scale 0"""
        sc, local = self.scale, self.local
        syn = [local[("syn", f, sc)].detach() for f in (-1, 1)] if ("syn", -1, sc) in local else None
        self._expose(out, dense, syn, local.get(("syn_region", sc)) if local.get(("syn_sparse", sc)) else None)


class TemporalLossStepFn(Function):
    """The step with the temporal hint (``--temporal``, loss_utils.py:84-88; ``--main_temporal``, :152-155): three library
    calls around the producer ``synth(inputs, outputs, scale) -> has_ins`` (upstream: dyn_utils.image_synthesis), which
    reads a pass's warped images ``outputs[("color", f, 0)]`` and writes ``outputs[("syn", f, 0)]`` with ordinary autograd
    ops (dyn_utils.py:127-128,145-146,163-168).  Forward: mal_loss_step_warp -> producer, once per hinted pass, the
    teacher's first as upstream calls them (recorded by autograd on a private copy of the warped images) ->
    mal_loss_step_fwd (hands back d loss / d syn); backward: the producer's own backward (torch.autograd.grad on that
    private graph), then mal_loss_step_bwd, whose gradient sweeps add what arrives through syn to d loss / d warped colour
    before the chain rule through the warp.  ``which`` = (teacher hinted, student hinted); ``expose`` = (mono_outputs, outputs)."""

    @staticmethod
    def forward(ctx, disp_t, disp_s, aa_m1, tr_m1, aa_p1, tr_p1, consts, cfg, synth, inputs, expose, which, ens_disp=None,
                scales=None):
        """``scales`` (--distil with sclm > 0): (sclm, teacher's ("disp", s) for s = 1..sclm, the student's) -- scale s of
        every hinted pass is warped by mal_loss_step_warp_scales and handed to the producer after scale 0 (_ScaleHint)"""
        consts, cfg = StepConsts(*consts), StepCfg(*cfg)
        a, keep, maps = _build_args(disp_t, disp_s, aa_m1, tr_m1, aa_p1, tr_p1, consts, cfg, temporal=which[0],
                                    main_temporal=which[1], ens_disp=ens_disp)
        B, _, H, W = keep.tens[0].shape
        dev = keep.tens[0].device
        hints = [_Hint(a, student, B, H, W, dev) for student, on in ((False, which[0]), (True, which[1])) if on]
        a.warp_sample_stride = 6 * H * W
        extra, sa, low = {h.student: [] for h in hints}, None, ()
        if scales is not None:
            sclm, low_t, low_s = scales
            sa = L.StepScalesArgs()
            sa.sclm = sclm
            low = [ops._req(t.detach(), "disp") for t in (*low_t, *low_s)]
            for s in range(1, sclm + 1):
                sa.disp_teacher[s], sa.disp_student[s] = low[s - 1].data_ptr(), low[sclm + s - 1].data_ptr()
            for h in hints:
                extra[h.student] = [_ScaleHint(sa, h.student, s, B, H, W, dev) for s in range(1, sclm + 1)]
        lib = L.load()
        L.check(lib.mal_loss_step_warp(C.byref(a)), "mal_loss_step_warp")
        try:  # the producer raised, or left something unusable: join what mal_loss_step_warp forked before the buffers are reused
            if sa is not None:
                L.check(lib.mal_loss_step_warp_scales(C.byref(a), C.byref(sa)), "mal_loss_step_warp_scales")
            for h in hints:
                if h.student:  # its warped images may have been written on the library's side stream
                    L.check(lib.mal_loss_step_student_ready(C.byref(a)), "mal_loss_step_student_ready")
                more = extra[h.student]
                h.produce(synth, inputs, defer=bool(more))
                if more:  # scales 1..sclm in upstream's order; the last call's answer stands for the pass (trainer.py:1162,1164)
                    for e in more:
                        e.produce(synth, inputs)
                    h.finish(has_ins=more[-1].has_ins)
        except BaseException:
            lib.mal_loss_step_abort(C.byref(a))
            raise
        L.check(lib.mal_loss_step_fwd(C.byref(a)), "mal_loss_step_fwd")
        ctx.hints, ctx.scale_hints = hints, (low, extra)  # the C structs hold their buffers' pointers
        for h in hints:
            for e in (h, *extra[h.student]):
                e.expose(expose[1] if h.student else expose[0], cfg.want_maps)
        return _end_fwd(ctx, a, keep, maps)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_total, *_):
        if g_total is None:
            return (None,) * TemporalLossStepFn.INPUTS[0]
        # option "tail_overlap": the backward chain (producer's backward -> teacher's gradient sweep) on the library's side
        # stream, behind the fused sweep only -- beside the epilogue and the reduction the forward left on this stream
        lib, a = L.load(), ctx.args
        side = C.c_void_p(0)
        L.check(lib.mal_loss_step_tail_begin(C.byref(a), C.byref(side)), "mal_loss_step_tail_begin")
        overlap = side.value is not None and side.value != a.stream
        ok = True
        try:
            for h in ctx.hints:
                ok = h.backward(stream=side.value if overlap else None) and ok
        finally:
            if side.value != a.stream and not (overlap and ok):  # nothing (or not everything) went there: join it back now
                L.check(lib.mal_loss_step_tail_cancel(C.byref(a)), "mal_loss_step_tail_cancel")
        return _run_bwd(ctx, g_total, TemporalLossStepFn)


TemporalLossStepFn.INPUTS = _input_positions(TemporalLossStepFn)


# ---------------------------------------------------------------------------------- input preparation of the one-call steps
def aug_keep(opt, outputs, B):
    """outputs["augmentation_mask"] (its first ``opt.batch_size`` rows) -> (keep, aug_is_mask): a contiguous float32 mask is
    passed as itself and 1 - mask is formed on the device; anything else as 1 - mask in float32"""
    aug = outputs["augmentation_mask"][:opt.batch_size]
    if aug.dtype == torch.float32 and aug.is_contiguous():
        return aug.reshape(B), True
    if not aug.is_floating_point():
        aug = aug.to(torch.float32)  # (a bool mask: torch refuses 1 - mask)
    return (1 - aug).to(torch.float32).reshape(B), False


def pose_leaves(mono_outputs):
    """axisangle_m1, translation_m1, axisangle_p1, translation_p1 out of ``mono_outputs``"""
    aa = [mono_outputs[("axisangle", 0, f)] for f in (-1, 1)]
    tr = [mono_outputs[("translation", 0, f)] for f in (-1, 1)]
    fix = lambda t: t[:, 0] if t.dim() == 4 else t  # the pose decoder emits (B,2,1,3); frame 0 of it is used
    return fix(aa[0]), fix(tr[0]), fix(aa[1]), fix(tr[1])


def draw_noise_maps(shape, dev, n, dead):
    """The tie-break noise of a step as ``config.noise_source`` says -> (n maps of ``shape``, None) or (None, philox seed).
    "philox": drawn inside the step's first kernel -- no RNG launch, no host work, no generator touched.  "cpu": the n maps,
    then ``dead`` more draws whose values nobody reads: the reference makes them (loss_utils.py:178 in compute_main_losses,
    trainer.py:1305-1308,1325 for the student's scales), so the global CPU generator stays on its stream.  "cuda": the n maps."""
    if config.noise_source == "philox":
        return None, config.noise_seed
    maps = [loss_utils.draw_noise(shape, dev) for _ in range(n)]
    if config.noise_source == "cpu":
        for _ in range(dead):
            torch.randn(shape)
    return maps, None


def loss_step(opt, inputs, mono_outputs, outputs, w_list=None, batch_size_scale=None, noise=None, want_maps=True,
              want_decisions=False, want_noise=False, image_synthesis=None):
    """process_batch's loss half in one call.  Reads the same dict entries as the reference:
    ``inputs[("color", f, 0)]``, ``("K", 0)``, ``("inv_K", 0)``; ``mono_outputs[("disp", 0)]``,
    ``("axisangle", 0, f)`` / ``("translation", 0, f)`` (networks/repdepth.py:155-156);
    ``outputs[("disp", 0)]``, ``"consistency_mask"``, ``"augmentation_mask"``, ``"lowest_cost"``.
    With ``opt.temporal`` the producer ``image_synthesis(inputs, outputs, scale) -> has_ins`` is called between the
    library calls (``TemporalLossStepFn``); ``mono_outputs`` then receives ``("color", f, 0)``, ``("syn", f, 0)`` and
    ``"has_ins"`` as the reference's generate_images_pred leaves them (trainer.py:1122-1125,1161-1165).
    ``opt.sclm`` 1..3 (``--scales 0 .. sclm``): ``("disp", s)`` is read from both dicts for s <= sclm; the losses read
    scale 0 only, so without a hint the result is the sclm = 0 step's and ``("disp", s > 0)`` gets no gradient; with one,
    the producer is also called on each scale's full-resolution warp (forward only), after scale 0 in upstream's order,
    ``("color", f, s)`` / ``("syn", f, s)`` are exposed, and the LAST call's answer decides whether scale 0's synthesised
    images join the min (trainer.py:1088-1165).  With
    ``opt.main_temporal`` (trainer.py:1164, loss_utils.py:152-155) it is called for the student's pass as well -- after the
    teacher's, as upstream -- and ``outputs`` receives the same keys and ``"multi_has_ins"``.
    Writes ``outputs["consistency_mask"]`` (x matching mask, trainer.py:592-593) when ``want_maps``.
    ``want_decisions`` (tests) adds ``maps["dec_teacher"]`` / ``["dec_student"]``: the per-pixel decisions of the two
    gradient passes (int32 (MAL_DEC_PLANES,B,H,W), include/mal_hip.h).
    Returns (losses dict, loss_list or None, maps dict)."""
    sclm = int(getattr(opt, "sclm", 0))
    if getattr(opt, "no_ssim", False) or not getattr(opt, "distil", True):
        # (--no_ssim is read by Trainer.compute_reprojection_loss, trainer.py:1217, i.e. on the non-distil route only: the
        # distillation losses call loss_utils.compute_reprojection_loss, :46-55, which has no such branch -- and Trainer.ssim
        # does not exist then, trainer.py:318)
        raise L.MalError("loss_step covers the --distil [--temporal] [--main_temporal] [--learn_ens] [--no_ens [--dual_distil]] "
                         "configuration; use MALLossPath.compute_batch_losses for no_ssim / non-distil runs")
    if sclm != 0:
        # --scales 0..sclm: the losses read scale 0 only (loss_utils.py:57-200); the other scales only warp and call the
        # temporal hint's producer (trainer.py:1088-1165), whose last answer decides
        why = ("v1_multiscale with sclm > 0" if getattr(opt, "v1_multiscale", False) else
               "sclm %d (0..%d)" % (sclm, L.MS_MAX_SCALES - 1) if not 0 < sclm < L.MS_MAX_SCALES else
               "frame_ids %s (only [0, -1, 1])" % (list(opt.frame_ids),) if list(opt.frame_ids) != [0, -1, 1] else None)
        H_, W_ = inputs[("color", 0, 0)].shape[-2:]
        if why is None and (H_ % (1 << sclm) or W_ % (1 << sclm)):
            why = "%dx%d not divisible by 2**sclm" % (H_, W_)
        if why is not None:
            raise L.MalError("loss_step with --distil covers sclm 1..%d with frames [0,-1,1] and sizes divisible by 2**sclm; "
                             "%s: use MALLossPath.compute_batch_losses" % (L.MS_MAX_SCALES - 1, why))
    ens_disp = None
    if getattr(opt, "learn_ens", False) and not getattr(opt, "no_ens", False):
        # the learnt ensemble head's disparity (loss_utils.py:240-241, trainer.py:596-597): warped by the ensemble pass,
        # distillation target where the ensemble wins, and a leaf that receives gradient there
        if "ens_disp" not in outputs:
            raise KeyError("opt.learn_ens reads outputs['ens_disp'] (the shipped RepDepth has no such head: the caller's network provides it)")
        ens_disp = outputs["ens_disp"]
    temporal, main_temporal = bool(getattr(opt, "temporal", False)), bool(getattr(opt, "main_temporal", False))
    if (temporal or main_temporal) and image_synthesis is None:
        raise L.MalError("loss_step with opt.temporal / opt.main_temporal needs image_synthesis(inputs, outputs, scale) -> has_ins "
                         "(upstream: dyn_utils.image_synthesis bound to the segmenter and the matcher, trainer.py:1161-1165)")
    color0 = inputs[("color", 0, 0)]
    B, _, H, W = color0.shape
    dev = color0.device
    scales = None
    if sclm:
        low = {}
        for name, d in (("mono_outputs", mono_outputs), ("outputs", outputs)):
            low[name] = [d[("disp", s)] for s in range(1, sclm + 1)]  # KeyError as upstream (trainer.py:1091)
            for s, t in enumerate(low[name], 1):
                if tuple(t.shape) != (B, 1, H >> s, W >> s) or t.dtype != torch.float32 or t.device != dev:
                    raise L.MalError("loss_step: %s[('disp', %d)] must be a float32 (B,1,H>>%d,W>>%d) = %s tensor on %s; got %s %s"
                                     % (name, s, s, s, (B, 1, H >> s, W >> s), dev, tuple(t.shape), t.dtype))
        scales = (sclm, low["mono_outputs"], low["outputs"])
    poses = pose_leaves(mono_outputs)
    if noise is not None and tuple(noise.shape) != (B, 1, H, W):
        raise L.MalError("loss_step: the tie-break noise must be (B,1,H,W) = %s; got %s" % ((B, 1, H, W), tuple(noise.shape)))
    philox = None
    if noise is None:  # (loss_utils.compute_mono_losses adds the noise whatever --disable_automasking says, loss_utils.py:105-106)
        drawn, seed = draw_noise_maps((B, 1, H, W), dev, 1, 1)
        noise, philox = (None, (seed, bool(want_noise))) if drawn is None else (drawn[0], None)
    keep, aug_is_mask = aug_keep(opt, outputs, B)
    blc = bool(getattr(opt, "loss_blc", False))
    w_main, w_distil = 1.0, 1.0
    if blc:
        scale = float(batch_size_scale if batch_size_scale is not None else opt.batch_size)
        w_main, w_distil = scale * float(w_list[0]), scale * float(w_list[1])
    consts = StepConsts(color0, inputs[("color", -1, 0)], inputs[("color", 1, 0)], inputs[("K", 0)], inputs[("inv_K", 0)],
                        outputs["consistency_mask"].to(torch.float32), keep, outputs["lowest_cost"], noise)
    cfg = StepCfg(opt.min_depth, opt.max_depth, bool(getattr(opt, "no_ens", False)), w_main, w_distil, bool(want_maps),
                  aug_is_mask, bool(want_decisions), philox, bool(getattr(opt, "dual_distil", False)))
    if temporal or main_temporal:
        res = TemporalLossStepFn.apply(mono_outputs[("disp", 0)], outputs[("disp", 0)], *poses, consts, cfg, image_synthesis,
                                       inputs, (mono_outputs, outputs), (temporal, main_temporal), ens_disp, scales)
    else:
        res = LossStepFn.apply(mono_outputs[("disp", 0)], outputs[("disp", 0)], *poses, consts, cfg, ens_disp)
    total, v = res[0].reshape(()), res[1]
    maps = dict(zip(map_names(cfg), res[2:]))
    if want_maps:
        outputs["consistency_mask"] = maps["consistency_mask"]
    losses = {"reproj_loss/0": v[V16.REPROJ_BOTH], "consistency_loss/0": v[V16.CONSISTENCY], "distil_loss": v[V16.DISTIL],
              "loss/0": v[V16.LOSS_BLC] if blc else v[V16.LOSS_PLAIN], "loss": total, "mono/reproj_loss/0": v[V16.REPROJ_T],
              "mono/loss": v[V16.LOSS_T], "smooth_loss/mono": v[V16.SMOOTH_T], "smooth_loss/multi": v[V16.SMOOTH_S],
              "main/reproj_loss/0": v[V16.REPROJ_S]}
    loss_list = [v[V16.LOSS_BLC], v[V16.DISTIL]] if blc else None
    return losses, loss_list, maps


_CAPTURE = None  # teacher_pass_replay: receives (argument block, kept tensors) of the next LossStepFn.forward


def teacher_pass_replay(opt, inputs, mono_outputs, outputs, **kw):
    """Measurement hook (bench.py's ``roofline`` block).  Runs ONE forward of the step without the temporal hint on the
    given dicts (so the workspace holds the texels, the identity map and the camera block) and returns
    ``enqueue(launches)``: each call enqueues that many back-to-back launches of the teacher's pass -- the fused
    warp + SSIM + L1 + min + automask forward+backward sweep -- on the current stream, with the argument block of that
    forward (``mal_loss_step_teacher_replay``).  Capture ``enqueue(64)`` into a graph, replay it, time it with two events
    outside the graph: the kernel alone, as a replayed step runs it."""
    global _CAPTURE
    import copy
    o = copy.copy(opt)
    o.temporal = False
    _CAPTURE = []
    try:
        with torch.no_grad():
            loss_step(o, inputs, mono_outputs, outputs, want_maps=False, **kw)
        got = list(_CAPTURE)
    finally:
        _CAPTURE = None
    a, keep = got[0]

    def enqueue(launches):
        a.stream = ops._stream()
        L.check(L.load().mal_loss_step_teacher_replay(C.byref(a), int(launches)), "mal_loss_step_teacher_replay")

    enqueue.keep = keep  # the block holds raw pointers
    return enqueue


# ---------------------------------------------------------------------------------- sclm > 0, no --distil
class MultiScaleLossFn(Function):
    """leaves: disp_teacher[0..sclm], disp_student[0..sclm], axisangle_m1, translation_m1, axisangle_p1, translation_p1"""

    @staticmethod
    def forward(ctx, consts, cfg, *leaves):
        consts, cfg = MsConsts(*consts), MsCfg(*cfg)
        colors, colors_s, K, inv_K, cmask, keep, lowest, noises = consts
        sclm, philox, hint = cfg.sclm, cfg.philox, cfg.hint
        S = sclm + 1
        if noises is not None and len(noises) != S:
            raise L.MalError("MultiScaleLossFn: one noise map per scale (%d), or None; got %d" % (S, len(noises)))
        req, p = ops._req, ops._p
        tens = [req(t, "leaf") for t in leaves]
        cons = [req(t, "input") for t in (*colors, *colors_s, K, inv_K, cmask, keep)]
        cons += [None if t is None else req(t, "input") for t in (lowest, *(noises or ()))]
        B, _, H, W = tens[0].shape
        dev = tens[0].device
        for s in range(S):
            for t in (tens[s], tens[S + s]):
                if tuple(t.shape) != (B, 1, H >> s, W >> s):
                    raise L.MalError("loss_step_multiscale: the disparity of scale %d must be (B,1,%d,%d)" % (s, H >> s, W >> s))
        a = L.MsArgs()
        a.B, a.H, a.W, a.sclm = B, H, W, sclm
        a.min_depth, a.max_depth = float(cfg.min_depth), float(cfg.max_depth)
        a.flags = (L.STEP_AUG_MASK if cfg.aug_is_mask else 0) | (L.STEP_NO_SSIM if cfg.no_ssim else 0) | int(cfg.extra_flags)
        a.color0, a.color_m1, a.color_p1 = (p(t) for t in cons[:3])
        for s in range(1, S):
            a.color0_s[s] = p(cons[3 + s - 1])
        o = 3 + sclm
        a.K, a.inv_K, a.consistency_mask, a.augmentation_keep = (p(t) for t in cons[o:o + 4])
        a.lowest_cost = p(cons[o + 4])
        for s in range(S):
            a.disp_teacher[s], a.disp_student[s] = p(tens[s]), p(tens[S + s])
            if noises is not None:
                a.noise[s] = p(cons[o + 5 + s])
        a.axisangle_m1, a.translation_m1, a.axisangle_p1, a.translation_p1 = (p(t) for t in tens[2 * S:])
        if philox is not None:
            a.flags |= L.STEP_NOISE_PHILOX
            a.noise_seed = int(philox) & 0xFFFFFFFFFFFFFFFF
            a.noise_counter = noise_counter(dev).data_ptr()
        losses = torch.empty(48, dtype=torch.float32, device=dev)
        total = torch.empty(1, dtype=torch.float32, device=dev)
        a.losses, a.loss_total = p(losses), p(total)
        outs = [total, losses]
        if cfg.want_maps and lowest is not None and not (a.flags & L.STEP_NO_MOTION_MASK):
            cm = torch.empty((B, H, W), dtype=torch.float32, device=dev)
            a.consistency_mask_out = p(cm)
            outs.append(cm)
        decs = []
        if cfg.want_decisions:  # one (MAL_DEC_PLANES,B,H,W) int32 block per network and scale (include/mal_hip.h MAL_DEC_*)
            decs = [torch.zeros((L.DEC_PLANES, B, H, W), dtype=torch.int32, device=dev) for _ in range(2 * S)]
            for s in range(S):
                a.dec_teacher[s], a.dec_student[s] = p(decs[s]), p(decs[S + s])
            outs += decs
        ctx.n_dec = len(decs)
        ws = byte_workspace("multiscale", dev, L.load().mal_ms_workspace_bytes(B, H, W, sclm), B, H, W, sclm)
        a.ws, a.ws_bytes, a.stream = p(ws), ws.numel(), ops._stream()
        hints = []
        if hint is not None:
            # the temporal hint on this path (trainer.py:1161-1162,1279-1283): the producer once per scale, on that scale's
            # full-resolution warp of the teacher, between mal_loss_multiscale_warp and _fwd; has_ins is the LAST call's
            synth, inputs, expose = hint
            a.flags |= L.STEP_TEMPORAL
            a.warp_sample_stride = 6 * H * W
            hints = [_Hint(a, False, B, H, W, dev, scale=s_) for s_ in range(S)]
            L.check(L.load().mal_loss_multiscale_warp(C.byref(a)), "mal_loss_multiscale_warp")
            try:  # a producer raised, or left something unusable: join what _warp forked before the buffers are reused
                for h in hints:
                    h.produce(synth, inputs, defer=True)
                has_ins = hints[-1].has_ins
                for h in hints:
                    h.finish(has_ins)
            except BaseException:
                L.load().mal_loss_multiscale_abort(C.byref(a))
                raise
        L.check(L.load().mal_loss_multiscale_fwd(C.byref(a)), "mal_loss_multiscale_fwd")
        for h in hints:
            h.expose(hint[2], cfg.want_maps)
        ctx.hints = hints  # the argument block holds their buffers' pointers
        ctx.args, ctx.keep, ctx.S = a, Kept(tens, cons, ws, losses, total), S
        ctx.ws_token = ops.claim_workspace(ws)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*outs[1:])
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_total, *_):
        tens, S = ctx.keep.tens, ctx.S
        if g_total is None:
            return (None,) * (2 + len(tens))
        ops.check_workspace(ctx.keep.ws, ctx.ws_token, "loss_step_multiscale backward")
        g_total = g_total.reshape(1).contiguous()
        a = ctx.args
        grads = [torch.empty_like(t) if ctx.needs_input_grad[2 + i] else None for i, t in enumerate(tens)]
        a.g_total = ops._p(g_total)
        for s in range(S):
            a.g_disp_teacher[s], a.g_disp_student[s] = ops._p(grads[s]), ops._p(grads[S + s])
        a.g_axisangle_m1, a.g_translation_m1, a.g_axisangle_p1, a.g_translation_p1 = (ops._p(g) for g in grads[2 * S:])
        for h in ctx.hints:
            h.backward()  # the producer's own backward: g_syn -> g_warp of that scale
        L.check(L.load().mal_loss_multiscale_bwd(C.byref(a)), "mal_loss_multiscale_bwd")
        return (None, None, *grads)


def loss_step_multiscale(opt, inputs, mono_outputs, outputs, noises=None, want_maps=True, image_synthesis=None,
                         want_decisions=False):
    """process_batch's loss half WITHOUT ``--distil`` (manydepth/trainer.py:573-612 with ``compute_losses``, :1248-1475,
    for both networks) over scales 0..``opt.sclm`` in one call per direction.  Reads ``inputs[("color", f, 0)]``,
    ``("color", 0, s)``, ``("K", 0)``, ``("inv_K", 0)``; ``mono_outputs[("disp", s)]``, ``("axisangle", 0, f)``,
    ``("translation", 0, f)``; ``outputs[("disp", s)]``, ``"consistency_mask"``, ``"augmentation_mask"`` and, when present,
    ``"lowest_cost"`` (then the matching mask of trainer.py:592-593 is applied and ``outputs["consistency_mask"]``
    rewritten).  ``noises``: one (B,1,H,W) N(0,1) map per scale (default: drawn as ``config.noise_source`` says).
    With ``opt.temporal`` the producer ``image_synthesis(inputs, outputs, scale) -> has_ins`` is called once per scale on the
    teacher's full-resolution warp of that scale (trainer.py:1161-1162) and, when the LAST call reported instances, every
    scale's min takes the two synthesised candidates in (:1279-1283; a scale whose own call reported none then raises the
    ``KeyError`` upstream raises); ``mono_outputs`` receives ``("color", f, s)``, ``("syn", f, s)`` and ``"has_ins"``.
    Returns (losses, mono_losses): ``losses`` as process_batch leaves it (the teacher's entries added to the
    student's, :614-616; ``losses["loss"]`` carries the gradient), ``mono_losses`` the teacher's own.
    ``want_decisions`` (tests): a third value ``{"dec_teacher": [per scale], "dec_student": [per scale]}`` -- the per-pixel
    decisions of every scale's gradient passes (int32 (MAL_DEC_PLANES,B,H,W) each, include/mal_hip.h)."""
    sclm = int(getattr(opt, "sclm", 0))
    temporal = bool(getattr(opt, "temporal", False))
    if noises is not None and len(noises) != sclm + 1:
        raise L.MalError("loss_step_multiscale: `noises` holds one map per scale 0..%d; got %d" % (sclm, len(noises)))
    if temporal and image_synthesis is None:
        raise L.MalError("loss_step_multiscale with opt.temporal needs image_synthesis(inputs, outputs, scale) -> has_ins")
    unsupported = [k for k in ("distil", "v1_multiscale") if getattr(opt, k, False)]
    if getattr(opt, "no_ssim", False) and getattr(opt, "temporal", False):
        unsupported.append("no_ssim with temporal")
    if unsupported or sclm >= L.MS_MAX_SCALES or list(opt.frame_ids) != [0, -1, 1]:
        # (--v1_multiscale with sclm > 0 cannot run upstream for the student either: its (B,1,H>>s,W>>s) mask is multiplied
        # by the full-resolution consistency mask, manydepth/trainer.py:1322)
        raise L.MalError("loss_step_multiscale covers the non-distil sclm <= 3 configuration with frames [0,-1,1]; %s: use "
                         "MALLossPath.compute_batch_losses" % (", ".join(unsupported) or "this configuration"))
    color0 = inputs[("color", 0, 0)]
    B, _, H, W = color0.shape
    dev = color0.device
    poses = pose_leaves(mono_outputs)
    philox = None
    if getattr(opt, "disable_automasking", False):
        noises = None  # upstream still compares against the identity term (trainer.py:1296-1311): only the tie-break noise goes
    elif noises is None:
        noises, philox = draw_noise_maps((B, 1, H, W), dev, sclm + 1, sclm + 1)
    keep, aug_is_mask = aug_keep(opt, outputs, B)
    consts = MsConsts((color0, inputs[("color", -1, 0)], inputs[("color", 1, 0)]),
                      [inputs[("color", 0, s)] for s in range(1, sclm + 1)], inputs[("K", 0)], inputs[("inv_K", 0)],
                      outputs["consistency_mask"].to(torch.float32), keep, outputs.get("lowest_cost"), noises)
    cfg = MsCfg(opt.min_depth, opt.max_depth, sclm, aug_is_mask, philox, bool(want_maps),
                hint=(image_synthesis, inputs, mono_outputs) if temporal else None, no_ssim=bool(getattr(opt, "no_ssim", False)),
                extra_flags=(L.STEP_NO_MOTION_MASK if getattr(opt, "disable_motion_masking", False) else 0) |
                (L.STEP_NO_AUG if getattr(opt, "no_matching_augmentation", False) else 0) |
                (L.STEP_ENSEMBLE if getattr(opt, "ensemble", False) else 0), want_decisions=bool(want_decisions))
    leaves = [mono_outputs[("disp", s)] for s in range(sclm + 1)] + [outputs[("disp", s)] for s in range(sclm + 1)]
    res = MultiScaleLossFn.apply(consts, cfg, *leaves, *poses)
    total, v = res[0].reshape(()), res[1]
    n_dec = 2 * (sclm + 1) if want_decisions else 0
    decs = res[len(res) - n_dec:] if n_dec else ()
    if len(res) - n_dec > 2:
        outputs["consistency_mask"] = res[2]
    elif want_maps and outputs.get("lowest_cost") is not None and getattr(opt, "disable_motion_masking", False):
        # process_batch multiplies the matching mask in whatever the loss does with it (trainer.py:592-593); the passes did not
        # form it (their weight leaves the mask out): one operator launch
        from . import layers
        with torch.no_grad():
            _, mono_depth = layers.disp_to_depth(mono_outputs[("disp", 0)].detach(), opt.min_depth, opt.max_depth)
            outputs["consistency_mask"] = ops.matching_mask(outputs["lowest_cost"], mono_depth[:, 0].contiguous(),
                                                            outputs["consistency_mask"].to(torch.float32))
    losses, mono_losses = {"loss": total}, {"loss": v[V48.TEACHER_TOTAL]}
    for s in range(sclm + 1):
        t, m = (lambda term: v[V48.at(V48.TEACHER, s, term)]), (lambda term: v[V48.at(V48.STUDENT, s, term)])
        losses["reproj_loss/%d" % s], losses["loss/%d" % s] = v[V48.REPROJ_BOTH + s], v[V48.LOSS_BOTH + s]
        losses["consistency_loss/%d" % s] = m(V48.CONSISTENCY)
        losses["main/reproj_loss/%d" % s], losses["main/loss/%d" % s] = m(V48.REPROJ), m(V48.LOSS)
        losses["smooth_loss/multi/%d" % s], mono_losses["smooth_loss/%d" % s] = m(V48.SMOOTH), t(V48.SMOOTH)
        if getattr(opt, "ensemble", False):
            losses["ensemble_loss/%d" % s] = v[V48.ENSEMBLE + s]
        mono_losses["reproj_loss/%d" % s], mono_losses["loss/%d" % s] = t(V48.REPROJ), t(V48.LOSS)
    losses["main/loss"] = v[V48.STUDENT_TOTAL]
    if want_decisions:
        return losses, mono_losses, {"dec_teacher": list(decs[:sclm + 1]), "dec_student": list(decs[sclm + 1:])}
    return losses, mono_losses
