"""GPU: the decoder glue (mal_amd/csrc/mal_glue.hip) and the encoder glue (mal_amd/csrc/mal_bn.hip) over the tables of
tests/glue_sweep_cases.py, under the rules of tests/test_gpu_decoder_glue.py and the gates of tests/test_gpu_encoder_glue.py.
tests/test_glue_sweep_cases.py shows on the CPU which band each case fills.  No tolerance is new.

Decoder glue, every case strided over the capped grid or ending inside a thread's unit of 4 floats:
  forward    the int32 words of ATen's composition on the device; where ATen has a NaN, a NaN (x carries +-inf, both smallest
             denormals, -1e-8, -88.8, -104 and a NaN besides the planted values of the old table)
  backward   |got - exact| <= n * 2^-24 * |a'| * sum|terms| per element.  The exact sums, sum|terms| and the term counts n are
             torch.autograd of the composition WITHOUT the activation in fp64 on the device, applied to g, |g| and ones (the
             restatement's einsum is too slow at 9 M elements; tests/test_decoder_glue_cases.py ties the two).  fp64 sums of at
             most 16 terms are within 2^-49 sum|terms| of exact, 2^-25 of the smallest bound.  a' is the fp32 factor y + 1 of
             the forward's own output.  Finite inputs only.  ATen's own backward is held to twice the bound
  pruning    gx alone and gskip alone are the full call's bits (the grid changes with the larger output, the order does not)
  repeat     a second call gives the same bits
  placement  out, gx, gskip written and x read 0..3 floats off the 16-byte grid, through the C entry points into windows of
             larger buffers prefilled with a bit pattern: the window holds the aligned call's bits, 64 guard words on either
             side keep the pattern; and x as a contiguous view at storage offset 1 through decoder_join itself

Encoder glue: the 4-byte route by placement (x, residual, cotangent 1..3 floats into a buffer) on both sides of every change
of blocks per channel, the eval-mode kernel over the whole table, every subset of the requested gradients, expanded /
channels-last / sliced cotangents, a captured training step replayed on rewritten inputs, and inputs of mean 4096 and
std 1/64 -- all through evaluate() and the hold_* gates of tests/test_gpu_encoder_glue.py.

With MAL_GLUE_SWEEP_REPORT=<file> the worst error / bound of the decoder's backward, the worst distance / gate of each
batch-norm quantity per case and the wall time of this file are written there."""
import functools
import os
import time

import pytest
import torch
import torch.nn.functional as F

from tests import decoder_glue_restated as R
from tests import encoder_glue_cases as E
from tests import glue_sweep_cases as G
from tests import test_gpu_decoder_glue as TD
from tests import test_gpu_encoder_glue as TE

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
PATTERN = 0x7FA5C3E1  # no value any of the kernels computes here: a NaN with a payload
GUARD = 64
REPORT, T0 = [], time.time()
STRIDED_IDS = {case: band for band, case in G.STRIDED.items()}


def did(case):
    return (STRIDED_IDS[case] + "-" if case in STRIDED_IDS else "tail-") + R.case_id(case)


@pytest.fixture(scope="module", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("MAL_GLUE_SWEEP_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("".join(REPORT) + "wall time of tests/test_gpu_glue_sweep.py: %.1f s\n" % (time.time() - T0))


def note(op, case, text):
    REPORT.append("%-14s %-84s %s\n" % (op, case, text))


def dev():
    return torch.device("cuda:0")


# ========================================================================================================== decoder glue
@functools.lru_cache(None)
def decoder_inputs(case, nonfinite):
    """(x, skip or None, g) on the device, made once per case and never written"""
    return tuple(None if a is None else torch.from_numpy(a).to(dev()) for a in G.decoder_inputs(case, nonfinite=nonfinite))


def same_words(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("case", G.SWEEP_CASES, ids=did)
def test_forward_is_bit_equal_to_aten(case):
    from mal_amd.glue import decoder_join
    up, elu, B, C, Cs, h, w = case
    x, skip, g = decoder_inputs(case, True)
    got = decoder_join(x, skip, up=up, elu=bool(elu))
    ref = TD.aten_composition(x, skip, up, elu)
    assert got.shape == ref.shape == (B, C + Cs, up * h + 2, up * w + 2) and got.is_contiguous()
    nan = torch.isnan(ref)
    assert bool(nan.any()) == bool(torch.isnan(x).any())
    assert torch.equal(torch.isnan(got), nan)  # a NaN where ATen has one; the payloads are not compared
    assert torch.equal(got.view(torch.int32).masked_fill(nan, 0), ref.view(torch.int32).masked_fill(nan, 0)), \
        float((got - ref).nan_to_num(0.0, 0.0, 0.0).abs().max())
    assert same_words(decoder_join(x, skip, up=up, elu=bool(elu)), got)  # the same bits again, NaN payloads included


def exact_sums(gm, case):
    """autograd of the composition without the activation, in the dtype of gm (fp64): what each element of gx and gskip sums"""
    up, elu, B, C, Cs, h, w = case
    zx = torch.zeros(B, C, h, w, dtype=gm.dtype, device=gm.device, requires_grad=True)
    zs = torch.zeros(B, Cs, up * h, up * w, dtype=gm.dtype, device=gm.device, requires_grad=True) if Cs else None
    TD.aten_composition(zx, zs, up, 0).backward(gm)
    return zx.grad, (zs.grad if Cs else None)


def held(got, exact, bound, what):
    err = (got.double() - exact).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(what, "max err / bound %.3f" % ratio)
    assert bool((err <= bound).all()), (what, ratio)
    return ratio


@pytest.mark.parametrize("case", G.SWEEP_CASES, ids=did)
def test_backward_within_the_derived_bound(case):
    from mal_amd.glue import decoder_join, decoder_join_bwd
    up, elu, B, C, Cs, h, w = case
    x, skip, g = decoder_inputs(case, False)
    assert bool(torch.isfinite(x).all())
    lx = x.clone().requires_grad_(True)
    ls = skip.clone().requires_grad_(True) if Cs else None
    out = decoder_join(lx, ls, up=up, elu=bool(elu))
    out.backward(g)
    g64 = g.double()
    sx, ss = exact_sums(g64, case)
    ax, as_ = exact_sums(g64.abs(), case)
    nx, ns = exact_sums(torch.ones_like(g64), case)
    assert float(nx.min()) >= 1 and float(nx.max()) <= 16 and bool((nx == nx.round()).all())
    if elu:  # the fp32 factor of the forward's own output: the decision x > 0 is thereby forced
        y = out.detach()[:, :C, 1:-1:up, 1:-1:up]
        assert y.shape == x.shape
        a = torch.where(y > 0, torch.ones_like(y), y + 1.0).double()
        sx, bx = a * sx, nx * U * a.abs() * ax
    else:
        bx = nx * U * ax
    name = did(case)
    rx = held(lx.grad, sx, bx, name + " gx")
    rs = held(ls.grad, ss, ns * U * as_, name + " gskip") if Cs else 0.0
    note("decoder_join", name, "backward: worst error / bound gx %.3f gskip %.3f" % (rx, rs))
    # ATen's own backward on the device (atomics, another order): twice the bound
    tx = x.clone().requires_grad_(True)
    ts = skip.clone().requires_grad_(True) if Cs else None
    TD.aten_composition(tx, ts, up, elu).backward(g)
    assert bool(((tx.grad.double() - sx).abs() <= 2 * bx).all())
    if Cs:
        assert bool(((ts.grad.double() - ss).abs() <= 2 * ns * U * as_).all())
    # pruned and repeated calls: the same bits
    xin, shape = (x if elu else None), tuple(x.shape)
    only_x, none_s = decoder_join_bwd(g, xin, Cs, up, bool(elu), need_x=True, need_skip=False, shape=shape)
    assert none_s is None and same_words(only_x, lx.grad)
    again_x, again_s = decoder_join_bwd(g, xin, Cs, up, bool(elu), need_x=True, need_skip=True, shape=shape)
    assert same_words(again_x, lx.grad)
    if Cs:
        none_x, only_s = decoder_join_bwd(g, xin, Cs, up, bool(elu), need_x=False, need_skip=True, shape=shape)
        assert none_x is None and same_words(only_s, ls.grad) and same_words(again_s, ls.grad)


# ---- placement: windows into larger buffers, through the C entry points
def window(n, off):
    """(the whole buffer as int32, n floats of it that start GUARD + off floats in): prefilled, guards on both sides"""
    buf = torch.full((n + 2 * GUARD + 4,), PATTERN, dtype=torch.int32, device=dev())
    assert buf.data_ptr() % 16 == 0
    return buf, buf.view(torch.float32)[GUARD + off:GUARD + off + n]


def guards_kept(buf, n, off):
    return bool((buf[:GUARD + off] == PATTERN).all()) and bool((buf[GUARD + off + n:] == PATTERN).all())


PLACED_DECODER = G.TAILS + [G.STRIDED["gx_and_gskip_strided"]]


@pytest.mark.parametrize("case", PLACED_DECODER, ids=did)
def test_forward_into_an_unaligned_window(case):
    from mal_amd import _lib as L
    from mal_amd.glue import decoder_join_fwd
    from mal_amd.ops import _p, _stream
    up, elu, B, C, Cs, h, w = case
    x, skip, g = decoder_inputs(case, True)
    want = decoder_join_fwd(x, skip, up, bool(elu))
    n = want.numel()
    for off in range(4):
        buf, win = window(n, off)
        assert (win.data_ptr() % 16 == 0) == (off == 0)
        L.check(L.load().mal_decoder_join_fwd(_p(x), _p(skip), _p(win), B, C, Cs, h, w, up, elu, _stream()), "mal_decoder_join_fwd")
        torch.cuda.synchronize()
        assert guards_kept(buf, n, off), off
        assert same_words(win, want.view(-1)), off  # the access width does not enter the arithmetic


@pytest.mark.parametrize("case", PLACED_DECODER, ids=did)
def test_backward_with_unaligned_windows(case):
    from mal_amd import _lib as L
    from mal_amd.glue import decoder_join_bwd
    from mal_amd.ops import _p, _stream
    up, elu, B, C, Cs, h, w = case
    x, skip, g = decoder_inputs(case, False)
    want_x, want_s = decoder_join_bwd(g, x if elu else None, Cs, up, bool(elu), shape=tuple(x.shape))
    nx, ns = x.numel(), (want_s.numel() if Cs else 0)
    for which in ("x", "gx", "gskip"):
        if (which == "x" and not elu) or (which == "gskip" and not Cs):
            continue
        for off in range(4):
            ox, ogx, ogs = (off if which == k else 0 for k in ("x", "gx", "gskip"))
            xin = G.placed(x, ox) if elu else None
            bx, wx = window(nx, ogx)
            bs, ws = window(ns, ogs) if Cs else (None, None)
            L.check(L.load().mal_decoder_join_bwd(_p(g), _p(xin), _p(wx), _p(ws), B, C, Cs, h, w, up, elu, _stream()), "mal_decoder_join_bwd")
            torch.cuda.synchronize()
            assert guards_kept(bx, nx, ogx), (which, off)
            assert same_words(wx, want_x.view(-1)), (which, off)
            if Cs:
                assert guards_kept(bs, ns, ogs), (which, off)
                assert same_words(ws, want_s.view(-1)), (which, off)
    # one output alone, into a window: the other pointer is null
    for off in (1, 3):
        bx, wx = window(nx, off)
        L.check(L.load().mal_decoder_join_bwd(_p(g), _p(x if elu else None), _p(wx), None, B, C, Cs, h, w, up, elu, _stream()), "mal_decoder_join_bwd")
        torch.cuda.synchronize()
        assert guards_kept(bx, nx, off) and same_words(wx, want_x.view(-1))


@pytest.mark.parametrize("case", [G.TAILS[-1], G.STRIDED["gx_and_gskip_strided"]], ids=did)
def test_x_as_a_view_at_storage_offset_one(case):
    from mal_amd.glue import decoder_join
    up, elu, B, C, Cs, h, w = case
    assert elu and Cs
    x, skip, g = decoder_inputs(case, False)
    res = []
    for off in (0, 1):
        lx = G.placed(x, off).requires_grad_(True)
        ls = skip.clone().requires_grad_(True)
        assert lx.is_contiguous() and lx.storage_offset() == off
        out = decoder_join(lx, ls, up=up, elu=True)
        out.backward(g)
        res.append((out.detach(), lx.grad, ls.grad))
    for a, b in zip(*res):
        assert same_words(a, b)


# ========================================================================================================== encoder glue
def hold_record(case, rec, tag):
    assert rec["deterministic"]
    worst = dict(TE.hold_forward(case, rec))
    worst.update(TE.hold_module_state(case, rec))
    worst.update(TE.hold_backward(case, rec))
    note("bn_join", "%s %s" % (E.case_id(case), tag), "distance / gate: " + " ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    return worst


def _placed_cases():
    out = []
    for shape in G.placed_shapes():
        out += [((shape, "residual_relu", 0.0), place) for place in G.PLACEMENTS]
        out += [((shape, "plain", 100.0), place) for place in ((1, 0, 0), (0, 0, 3))]  # no ReLU: the output is not read back
    return out


@pytest.mark.parametrize("case,place", _placed_cases(), ids=lambda v: E.case_id(v) if len(v) == 3 and isinstance(v[0], tuple) else "x%d_r%d_g%d" % v)
def test_operands_off_the_16_byte_grid(case, place):
    """H*W % 4 == 0, so the 4-byte route is taken for the addresses alone; (0, 0, g): a 16-byte forward, a 4-byte backward.
    Against the aligned run only the gates hold, not the bits: the group-of-4 merge differs"""
    hold_record(case, TE.evaluate(case, place), "placed x+%d r+%d g+%d" % place)


@pytest.mark.parametrize("case", G.OFFSET_CASES, ids=E.case_id)
def test_offset_statistics(case):
    """mean 4096, std 1/64: the variance is 1.5e-11 of the second moment"""
    hold_record(case, TE.evaluate(case, (0, 0, 0), G.offset_inputs), "std 1/64")


def _eval_cases():
    return [(s, m, 0.0) for s in E.TABLE_SHAPES + E.boundary_shapes()[:2] for m in E.MODES]


@pytest.mark.parametrize("case", _eval_cases(), ids=E.case_id)
def test_eval_mode_kernel(case):
    from mal_amd.glue import bn_join, bn_join_fallback_reason
    (B, C, H, W), mode, mean = case
    relu = E.relu_of(mode)
    x, r, g, gamma, beta, rm, rv = E.make_inputs(case)
    d = lambda t: None if t is None else t.to(dev())
    y64 = E.forward(x.double(), None if r is None else r.double(), gamma.double(), beta.double(), relu, rm.double(), rv.double())[0]
    bn, bn_a = (TE._module(C, gamma, beta, rm, rv, 0.1, dev()).eval() for _ in range(2))
    with torch.no_grad():
        assert bn_join_fallback_reason(d(x), bn, d(r)) is None
        y = bn_join(d(x), bn, d(r), relu)
        again = bn_join(d(x), bn, d(r), relu)
        ya = TE._aten(d(x), bn_a, d(r), relu)
    own, got = E.l2rel(ya, y64), E.l2rel(y, y64)
    gate = max(1e-6, 2 * own)
    print(E.case_id(case), "eval y %.3e ATen %.3e" % (got, own))
    note("bn_join", E.case_id(case) + " eval", "distance / gate: y %.3f" % (got / gate))
    assert got <= gate and y.grad_fn is None and torch.equal(y, again)
    assert torch.equal(bn.running_mean.cpu(), rm) and torch.equal(bn.running_var.cpu(), rv) and int(bn.num_batches_tracked) == 0


@pytest.mark.parametrize("mode", ["residual_relu", "plain"])
@pytest.mark.parametrize("shape", G.PRUNED_SHAPES + ["boundary"], ids=str)
def test_every_subset_of_the_gradients(shape, mode):
    from mal_amd.glue import bn_join, bn_join_bwd
    shape = E.boundary_shapes()[1] if shape == "boundary" else shape
    B, C, H, W = shape
    relu = E.relu_of(mode)
    x, r, g, gamma, beta, rm, rv = (None if t is None else t.to(dev()) for t in E.make_inputs((shape, mode, 0.0)))
    bn = TE._module(C, gamma, beta, rm, rv, 0.1, dev())
    y = bn_join(x.clone().requires_grad_(True), bn, r, relu)
    sx, sy, sw, sm, si = y.grad_fn.saved_tensors
    full = bn_join_bwd(g, sx, sy, sw, sm, si, relu)
    assert all(t is not None for t in full)
    for need in G.gradient_subsets():
        got = bn_join_bwd(g, sx, sy, sw, sm, si, relu, *need)
        for name, want, t, f in zip(("dx", "dr", "dgamma", "dbeta"), need, got, full):
            assert (t is not None) == want, (need, name)
            if want:
                assert same_words(t, f), (need, name)


@pytest.mark.parametrize("shape", [G.PLACED_SHAPE] + G.PRUNED_SHAPES, ids=str)
def test_cotangent_forms(shape):
    """autograd hands the node whatever it was given: an expanded scalar, another memory format, a strided slice"""
    from mal_amd.glue import bn_join
    B, C, H, W = shape
    case = (shape, "residual_relu", 0.0)
    x, r, g, gamma, beta, rm, rv = (t.to(dev()) for t in E.make_inputs(case))

    def run(cot):
        bn = TE._module(C, gamma, beta, rm, rv, 0.1, dev())
        lx, lr = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
        y = bn_join(lx, bn, lr, True)
        if cot is None:
            y.sum().backward()
        else:
            assert torch.equal(cot, cot.contiguous())
            y.backward(cot)
        return lx.grad, lr.grad, bn.weight.grad, bn.bias.grad

    ones = run(torch.ones(shape, device=dev()))
    for a, b in zip(run(None), ones):
        assert same_words(a, b)
    assert not torch.ones((), device=dev()).expand(shape).is_contiguous()
    for a, b in zip(run(torch.ones((), device=dev()).expand(shape)), ones):
        assert same_words(a, b)
    plain = run(g)
    wide = torch.zeros(B, C, H, 2 * W, device=dev())
    wide[..., ::2] = g
    forms = {"channels_last": g.to(memory_format=torch.channels_last), "slice": wide[..., ::2]}
    for name, cot in forms.items():
        assert not cot.is_contiguous(), name
        for a, b in zip(run(cot), plain):
            assert same_words(a, b), name


def test_training_step_replays_from_a_captured_graph():
    from mal_amd.glue import bn_join
    case = (G.PLACED_SHAPE, "residual_relu", 0.0)
    B, C, H, W = G.PLACED_SHAPE
    sets = [tuple(t.to(dev()) for t in E.make_inputs(case, seed=s)) for s in (0, 1, 2)]
    x, r, g, gamma, beta, rm, rv = sets[0]
    bn = TE._module(C, gamma, beta, rm, rv, 0.1, dev())
    sx, sr, sg = x.clone().requires_grad_(True), r.clone().requires_grad_(True), g.clone()
    hold = {}

    def one():
        sx.grad = sr.grad = bn.weight.grad = bn.bias.grad = None
        hold["y"] = bn_join(sx, bn, sr, True)
        hold["y"].backward(sg)

    side = torch.cuda.Stream()  # eager runs on a side stream first, as tests/test_gpu_decoder_glue.py captures
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one()
        one()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert int(bn.num_batches_tracked) == 2
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        one()
    torch.cuda.synchronize()
    assert int(bn.num_batches_tracked) == 2  # a capture runs nothing
    outs = (hold["y"], sx.grad, sr.grad, bn.weight.grad, bn.bias.grad)
    eager = TE._module(C, gamma, beta, rm, rv, 0.1, dev())  # the same module state, advanced by eager calls alone
    eager.load_state_dict(bn.state_dict())
    for k, (xi, ri, gi, *_) in enumerate((sets[1], sets[2]), 1):
        with torch.no_grad():
            sx.copy_(xi), sr.copy_(ri), sg.copy_(gi)
            for t in outs:
                t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        ex, er = xi.clone().requires_grad_(True), ri.clone().requires_grad_(True)
        eager.weight.grad = eager.bias.grad = None
        ey = bn_join(ex, eager, er, True)
        ey.backward(gi)
        for name, a, b in zip(("y", "dx", "dr", "dgamma", "dbeta"), outs, (ey, ex.grad, er.grad, eager.weight.grad, eager.bias.grad)):
            assert same_words(a.detach(), b.detach()), (k, name)
        assert int(bn.num_batches_tracked) == int(eager.num_batches_tracked) == 2 + k
        assert same_words(bn.running_mean, eager.running_mean) and same_words(bn.running_var, eager.running_var), k
