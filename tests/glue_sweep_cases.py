"""Tables and helpers of the glue sweep (tests/test_glue_sweep_cases.py on the CPU, tests/test_gpu_glue_sweep.py on the
device), importable without a device.  They extend the case tables the two glue families were merged with
(tests/decoder_glue_restated.py, tests/encoder_glue_cases.py) into the bands those tables do not reach.

Decoder glue (mal_amd/csrc/mal_glue.hip).  A launch is ``blocks`` workgroups of ``per`` floats of the flat output; the grid
is capped, and an output of more than ``blocks * per`` floats (one SWEEP) is strided over: every thread then carries its
(d0, d1, d2, d3) odometer across the grid stride with one conditional subtraction per digit (``odo_add`` below restates
the rule), the stride's digits computed on the host.  ``glue.decoder_join_plan`` says what the launches are; nothing here
restates the cap.  STRIDED names one shape per band, each the smallest found for its band; TAILS are small shapes whose flat
outputs end 1, 2 or 3 floats into a thread's unit of 4.  Cases are (up, elu, B, C, Cs, h, w) as in decoder_glue_restated.

Encoder glue (mal_amd/csrc/mal_bn.hip): placements of the operands 1 to 3 floats into a buffer (the 4-byte route V = 1 by
address alone), the subsets of the requested gradients, and one case of offset statistics (mean 4096, std 1/64)."""
import itertools

import numpy as np
import torch

from tests import decoder_glue_restated as R
from tests import encoder_glue_cases as E

# ---------------------------------------------------------------------------------------------------------- decoder glue
# band -> case.  What each band means is asserted from the plan in tests/test_glue_sweep_cases.py (band_of below).
STRIDED = {
    "fwd_exactly_one_sweep": (2, 1, 2, 40, 24, 63, 63),
    "fwd_one_sweep_and_a_short_tail": (2, 1, 1, 2, 1, 295, 590),
    "fwd_two_sweeps_every_stride_digit_nonzero": (2, 1, 3, 7, 5, 97, 171),
    "fwd_five_sweeps_leading_digit_zero_gx_strided_up2": (2, 1, 2, 11, 0, 300, 320),
    "gx_strided_up1": (1, 1, 2, 9, 0, 330, 357),
    "gskip_strided_gx_within_one_sweep": (2, 0, 2, 2, 7, 190, 200),
    "gx_and_gskip_strided": (1, 1, 2, 9, 9, 330, 357),
}
# the stride digits (d0, d1, d2, d3) of the forward's index space the table of the issue states, re-derived by the CPU test
STATED_FWD_DIGITS = {"fwd_two_sweeps_every_stride_digit_nonzero": (128, 20, 7, 2)}
# up = 1 and every extent from {1, 3, 5}: the products are odd, so these give the residues 1 and 3; a residue of 2 needs
# one even factor, and B = 2 is it.  The last three end inside a second workgroup.
TAILS = [
    (1, 1, 1, 1, 0, 3, 3),    # out 25 (1)   gx 9 (1)
    (1, 1, 1, 3, 0, 3, 3),    # out 75 (3)   gx 27 (3)
    (1, 1, 2, 1, 0, 3, 3),    # out 50 (2)   gx 18 (2)
    (1, 1, 1, 1, 1, 3, 3),    # out 50 (2)   gx 9 (1)    gskip 9 (1)
    (1, 0, 1, 1, 3, 3, 3),    # out 100 (0)  gx 9 (1)    gskip 27 (3)
    (1, 1, 2, 3, 1, 3, 5),    # out 280 (0)  gx 90 (2)   gskip 30 (2)
    (2, 1, 1, 3, 1, 3, 5),    # up = 2: out 384 (0), gx 45 (1), gskip 60 (0)
    (1, 1, 1, 3, 0, 19, 19),  # out 1323 (3) gx 1083 (3): the masked unit is in the second workgroup
    (1, 0, 1, 1, 3, 19, 19),  # gskip 1083 (3)
    (1, 1, 1, 5, 1, 19, 13),  # out 1890 (2) gx 1235 (3) gskip 247 (3)
]
SWEEP_CASES = list(STRIDED.values()) + TAILS
TRAINING_SHAPE = (2, 1, 12, 16, 0, 96, 320)  # the scale-0 join at B=12, 192x640: where the cap is read from
# written over x after decoder_glue_restated.PLANTED, in a second fixed scatter
DENORM = float(np.float32(2.0 ** -149))
PLANTED_FINITE = (DENORM, -DENORM, -1e-8, -88.8, -104.0)
PLANTED_NONFINITE = (float("inf"), float("-inf"), float("nan"))


def sizes(case):
    """elements of (out, gx, gskip)"""
    up, elu, B, C, Cs, h, w = case
    return B * (C + Cs) * (up * h + 2) * (up * w + 2), B * C * h * w, B * Cs * up * h * up * w


def spaces(case):
    """radices (r0, r1, r2) and elements of the three flat index spaces, as the entry points hand them to odo_space"""
    up, elu, B, C, Cs, h, w = case
    n_out, nx, ns = sizes(case)
    return {"out": ((up * w + 2, up * h + 2, C + Cs), n_out), "gx": ((w, h, C), nx), "gskip": ((up * w, up * h, max(Cs, 1)), ns)}


def plan(case, need_x=True, need_skip=True):
    """(blocks of the forward, blocks of the backward, floats per block), from the library"""
    from mal_amd.glue import decoder_join_plan
    up, elu, B, C, Cs, h, w = case
    return decoder_join_plan(B, C, Cs, h, w, up, need_x, need_skip)


def cap():
    """the largest grid the library launches: the plan of the training shape, which four times the batch does not raise"""
    up, elu, B, C, Cs, h, w = TRAINING_SHAPE
    blocks = plan(TRAINING_SHAPE)[0]
    assert plan((up, elu, 4 * B, C, Cs, h, w))[0] == blocks
    return blocks


def sweeps(n, blocks, per):
    return -(-n // (blocks * per)) if blocks else 0


def stride_digits(radices, blocks, per):
    """the digits of the grid's stride blocks * per over (r0, r1, r2), d3 unbounded: odo_space of the host code"""
    r0, r1, r2 = radices
    st = blocks * per
    return st % r0, st // r0 % r1, st // (r0 * r1) % r2, st // (r0 * r1 * r2)


def profile(case):
    """what the launches of a full call look like: per space (sweeps, stride digits), from the plan"""
    fwd, bwd, per = plan(case)
    out = {}
    for name, (radices, n) in spaces(case).items():
        blocks = fwd if name == "out" else bwd
        out[name] = (sweeps(n, blocks, per), stride_digits(radices, blocks, per))
    return out


def odo_of(flat, radices):
    r0, r1, r2 = radices
    return [flat % r0, flat // r0 % r1, flat // (r0 * r1) % r2, flat // (r0 * r1 * r2)]


def odo_add(o, stride, radices):
    """the carry rule of the kernels on numpy arrays of digits: each stride digit is below its radix, so a digit exceeds its
    radix by less than the radix and one conditional subtraction carries"""
    c = 0
    for k in range(3):
        o[k] = o[k] + stride[k] + c
        c = (o[k] >= radices[k]).astype(o[k].dtype)
        o[k] = o[k] - c * radices[k]
    o[3] = o[3] + stride[3] + c
    return o


def decoder_inputs(case, seed=0, nonfinite=True):
    """decoder_glue_restated.make_inputs with PLANTED_FINITE, and PLANTED_NONFINITE if asked for, written over further
    elements of x in a second fixed scatter (tensors of fewer elements than values take the first ones)"""
    x, skip, g = R.make_inputs(case, seed)
    flat = x.reshape(-1)
    extra = PLANTED_FINITE + (PLANTED_NONFINITE if nonfinite else ())
    taken = {(k * 7919) % flat.size if flat.size >= len(R.PLANTED) else k for k in range(min(len(R.PLANTED), flat.size))}
    free = [i for i in ((3 + k * 104729) % flat.size for k in range(4 * len(extra))) if i not in taken]
    for i, v in zip(dict.fromkeys(free), extra):
        flat[i] = np.float32(v)
    return x, skip, g


# ---------------------------------------------------------------------------------------------------------- encoder glue
PLACED_SHAPE = (3, 64, 6, 20)
# floats (x, residual, cotangent) start into their buffers: each alone, all three, and the V = 4 forward with a V = 1 backward
PLACEMENTS = [(1, 0, 0), (0, 2, 0), (0, 0, 3), (1, 2, 3), (0, 0, 1)]
PRUNED_SHAPES = [(5, 3, 27, 33)]  # V = 1 by shape, more than one block per channel; one boundary shape joins it at run time
OFFSET_MEAN, OFFSET_STD = 4096.0, 1.0 / 64.0
OFFSET_CASES = [((3, 64, 6, 20), "residual_relu", OFFSET_MEAN), ((5, 3, 27, 33), "relu", OFFSET_MEAN)]


def placed_shapes():
    return E.boundary_shapes() + [PLACED_SHAPE]


def offset_inputs(case, seed=0):
    """encoder_glue_cases.make_inputs at mean 0 with x scaled to std OFFSET_STD and moved to the case's mean, the running
    mean moved with it (the constant channel stays constant)"""
    shape, mode, mean = case
    x, r, g, gamma, beta, rm, rv = E.make_inputs((shape, mode, 0.0), seed)
    x = (x.double() * OFFSET_STD + mean).float()
    return x, r, g, gamma, beta, (rm.double() + mean).float(), rv


def gradient_subsets():
    """every (need_x, need_r, need_w, need_b) but the empty one"""
    return [s for s in itertools.product((False, True), repeat=4) if any(s)]


def placed(t, offset, device=None):
    """a contiguous tensor of t's shape and values that starts ``offset`` floats into its own buffer"""
    device = t.device if device is None else device
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=device)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.storage_offset() == offset
    return view
