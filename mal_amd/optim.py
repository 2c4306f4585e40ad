"""``FlatAdam``: ``torch.optim.Adam`` (plain Adam, what upstream trains with: manydepth/trainer.py) over the
harness's flat gradient buffer as ONE HIP launch per step (mal_amd/csrc/mal_adam.hip, ``mal_adam_flat``).

The parameters stay where torch put them; a device-resident chunk table, built once, tells the kernel where every parameter
lives and where its gradient lies in ``FlatGradBucket.flat``.  ``exp_avg`` and ``exp_avg_sq`` are two flat buffers of the
optimizer's own with the bucket's offsets.  ``step(zero_grad=True)`` also zeroes the gradient buffer in the same pass (the
bucket's memset of the next step).  ``state_dict()`` / ``load_state_dict()`` speak ``torch.optim.Adam``'s format, so an
``adam.pth`` written by either optimizer loads into the other.

There is no CPU fallback: construction and the state dictionaries work on CPU tensors, ``step()`` raises ``MalError``.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L

_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable")


def adam_scalars(lr, beta1, beta2, eps, t):
    """the six kernel arguments of step ``t`` (>= 1), formed in double as ``torch.optim.Adam`` forms them (``_single_tensor_adam``)
    -> (c1, beta2, c2, bs, eps, a); ctypes rounds each to fp32 once"""
    step = float(t)
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    step_size = lr / bias_correction1
    bias_correction2_sqrt = bias_correction2 ** 0.5
    return 1 - beta1, beta2, 1 - beta2, bias_correction2_sqrt, eps, -step_size


def adam_plan(n_chunks, total_elements):
    """``mal_adam_plan`` (pure host code): {"blocks", "threads", "tile_elements", "table_window", "chunk_bytes"} of the launch
    ``mal_adam_flat`` makes for a range of ``n_chunks`` table entries with ``total_elements`` elements"""
    out = [ctypes.c_int(0) for _ in range(5)]
    L.check(L.load().mal_adam_plan(int(n_chunks), int(total_elements), *[ctypes.byref(o) for o in out]), "mal_adam_plan")
    return dict(zip(("blocks", "threads", "tile_elements", "table_window", "chunk_bytes"), (o.value for o in out)))


def _refuse(group):
    if group.get("weight_decay", 0) != 0:
        raise NotImplementedError("FlatAdam: weight_decay != 0 is not implemented (plain Adam only, as upstream trains)")
    for name in _UNSUPPORTED:
        if group.get(name, False):
            raise NotImplementedError("FlatAdam: %s is not implemented (plain Adam only, as upstream trains)" % name)


class FlatAdam(torch.optim.Optimizer):
    def __init__(self, params, bucket, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 capturable=False, differentiable=False):
        """``params``: the parameter list (no groups), the trainable ones in the order of ``bucket.params``; ``bucket``: the
        ``mal_amd.dp.FlatGradBucket`` that holds their gradients."""
        _refuse(dict(weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, capturable=capturable,
                     differentiable=differentiable))
        params = list(params)
        if any(isinstance(p, dict) for p in params):
            raise ValueError("FlatAdam: one parameter group only: pass the parameter list")
        params = [p for p in params if p.requires_grad]
        if len(params) != len(bucket.params) or any(a is not b for a, b in zip(params, bucket.params)):
            raise ValueError("FlatAdam: the parameters must be the bucket's, in its order")
        if bucket.flat.dtype != torch.float32:
            raise ValueError("FlatAdam: float32 parameters only, got %s" % bucket.flat.dtype)
        if bucket.flat.numel() >= 2 ** 31:
            raise ValueError("FlatAdam: %d elements; the kernel's offsets are 32-bit" % bucket.flat.numel())
        # torch's own group keys (whatever this torch build's Adam has), so schedulers and checkpoints see the usual group
        defaults = dict(torch.optim.Adam([torch.zeros(1)], lr=lr, betas=betas, eps=eps).defaults)
        super().__init__(params, defaults)
        self.bucket = bucket
        self._params = params
        self._counts = [p.numel() for p in params]
        self._offsets = [0]
        for n in self._counts[:-1]:
            self._offsets.append(self._offsets[-1] + n)
        self.exp_avg = torch.zeros_like(bucket.flat)
        self.exp_avg_sq = torch.zeros_like(bucket.flat)
        self.t = 0  # steps taken; every parameter's ``step`` in the state dictionary
        self._table, self._recorded = None, None

    # ---- the chunk table
    def _pointers(self):
        """(parameter pointers, gradient pointers) as they are now; a parameter without a gradient has None"""
        return ([p.data_ptr() for p in self._params],
                [p.grad.data_ptr() if p.grad is not None else None for p in self._params])

    def _build_table(self, pp):
        arr = (L.AdamChunk * len(pp))()
        for i, (ptr, off, n) in enumerate(zip(pp, self._offsets, self._counts)):
            arr[i].param, arr[i].offset, arr[i].count = ptr, off, n
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self._table = host.to(self.bucket.flat.device)
        self._recorded = list(pp)

    def _verify(self):
        """is the table still true?  A replaced parameter storage rebuilds it; a gradient that is no longer the bucket's view
        (``zero_grad(set_to_none=True)``, an assigned ``.grad``) cannot be mended from here"""
        pp, gp = self._pointers()
        base, es = self.bucket.flat.data_ptr(), self.bucket.flat.element_size()
        for i, (g, off) in enumerate(zip(gp, self._offsets)):
            if g != base + off * es:
                raise L.MalError("FlatAdam.step: the gradient of parameter %d is %s the bucket's view of the flat buffer (call "
                                 "bucket.zero_() or step(zero_grad=True), never zero_grad(set_to_none=True))"
                                 % (i, "missing, not" if g is None else "not"))
        if any(not p.is_contiguous() for p in self._params):
            raise L.MalError("FlatAdam.step: a parameter is no longer contiguous")
        if self._recorded != pp or self._table is None or self._table.device != self.bucket.flat.device:
            self._build_table(pp)

    # ---- the update
    @torch.no_grad()
    def step(self, closure=None, zero_grad=False):
        """one Adam update of every parameter: ONE launch on the current stream.  ``zero_grad``: the kernel overwrites each
        gradient element with 0 after reading it (the flat buffer is all zero afterwards)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_step()
        self.t += 1
        self.update_range(0, len(self._params), zero_grad, _checked=True)
        return loss

    def _check_step(self):
        _refuse(self.param_groups[0])
        flat = self.bucket.flat
        if not flat.is_cuda:
            raise L.MalError("FlatAdam.step: expected CUDA/HIP tensors, got %s (mal_amd has no CPU fallback)" % (flat.device,))
        self._verify()

    @torch.no_grad()
    def update_range(self, first, count, zero_grad=False, _checked=False):
        """the update of the parameters ``first .. first + count - 1`` (table entries) alone, at the CURRENT step number ``t``:
        a caller that cuts a step into ranges advances ``t`` once itself and sees that every entry is updated exactly once."""
        if not _checked:
            self._check_step()
        n = len(self._params)
        if first < 0 or count < 0 or first + count > n:
            raise L.MalError("FlatAdam.update_range: [%d, %d) is outside the %d parameters" % (first, first + count, n))
        group, flat = self.param_groups[0], self.bucket.flat
        beta1, beta2 = group["betas"]
        c1, b2, c2, bs, eps, a = adam_scalars(float(group["lr"]), beta1, beta2, group["eps"], max(self.t, 1))
        elements = sum(self._counts[first:first + count])
        with torch.cuda.device(flat.device):
            L.check(L.load().mal_adam_flat(self._table.data_ptr(), n, first, count, elements, flat.data_ptr(),
                                           self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), flat.numel(), self.t, c1, b2, c2,
                                           bs, eps, a, int(bool(zero_grad)), torch.cuda.current_stream().cuda_stream),
                    "mal_adam_flat")

    def zero_grad(self, set_to_none=False):
        """the gradients are views of the bucket's buffer and must stay so: always zeroes in place"""
        if set_to_none:
            raise ValueError("FlatAdam.zero_grad: set_to_none would drop the bucket's gradient views")
        self.bucket.zero_()

    # ---- torch.optim.Adam's checkpoint format
    def state_dict(self):
        """``torch.optim.Adam.state_dict()``'s layout: per parameter ``step`` (a float32 scalar, as torch keeps it), ``exp_avg``
        and ``exp_avg_sq`` as copies shaped like the parameter; before the first step the state is empty, as torch's"""
        sd = super().state_dict()  # the base class keeps no state of ours: param_groups packed as torch packs them
        state = {}
        if self.t > 0:
            for i, (p, off, n) in enumerate(zip(self._params, self._offsets, self._counts)):
                state[i] = {"step": torch.tensor(float(self.t), dtype=torch.float32),
                            "exp_avg": self.exp_avg[off:off + n].view_as(p).clone(),
                            "exp_avg_sq": self.exp_avg_sq[off:off + n].view_as(p).clone()}
        sd["state"] = state
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._params):
            raise ValueError("FlatAdam.load_state_dict: expected one group of %d parameters" % len(self._params))
        _refuse(groups[0])
        state = state_dict["state"]
        steps = set()
        if state:
            if sorted(state) != list(range(len(self._params))):
                raise ValueError("FlatAdam.load_state_dict: the state must cover every parameter or none")
            for i, p in enumerate(self._params):
                s = state[i]
                if "max_exp_avg_sq" in s:
                    raise NotImplementedError("FlatAdam: amsgrad is not implemented (the state has max_exp_avg_sq)")
                if tuple(s["exp_avg"].shape) != tuple(p.shape) or tuple(s["exp_avg_sq"].shape) != tuple(p.shape):
                    raise ValueError("FlatAdam.load_state_dict: the state of parameter %d has shape %s, the parameter %s"
                                     % (i, tuple(s["exp_avg"].shape), tuple(p.shape)))
                steps.add(float(s["step"]))
            if len(steps) != 1 or next(iter(steps)) != int(next(iter(steps))) or next(iter(steps)) < 0:
                raise ValueError("FlatAdam.load_state_dict: one whole step number for all parameters, got %s" % sorted(steps))
        for k, v in groups[0].items():
            if k != "params":
                self.param_groups[0][k] = v
        if not state:
            self.t = 0
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            return
        for i, (off, n) in enumerate(zip(self._offsets, self._counts)):
            self.exp_avg[off:off + n].copy_(state[i]["exp_avg"].reshape(-1))
            self.exp_avg_sq[off:off + n].copy_(state[i]["exp_avg_sq"].reshape(-1))
        self.t = int(next(iter(steps)))
