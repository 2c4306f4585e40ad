"""GPU: mal_amd.glue.decoder_join (mal_amd/csrc/mal_glue.hip) against the ATen composition it replaces and against the fp64
restatement (tests/decoder_glue_restated.py), DepthDecoder(fused_glue=True) against the unfused decoder, and the harness
with ``fused_decoder`` set.

Forward: torch.equal with F.pad(cat([interpolate(F.elu(x)), skip]), reflect) on the device -- copies admit nothing else, and
the negative ELU branch calls the same expm1 on float as ATen does.
Backward: |got - exact| <= n * 2^-24 * |a'| * sum|terms| per element, n the element's term count (n - 1 additions and one
product, each rounded once), exact = the fp64 restatement with the fp32 factor a' = y + 1 of the forward's own output
(the decision x > 0 is thereby forced).  ATen's own backward (atomics, another order) is held to twice that."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import decoder_glue_restated as R

pytestmark = pytest.mark.gpu
IDS = [R.case_id(c) for c in R.CASES]
U = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


def aten_composition(x, skip, up, elu):
    y = F.elu(x.clone(), inplace=True) if elu else x  # in place as ConvBlock does: its backward is g * (y + 1)
    if up == 2:
        y = F.interpolate(y, scale_factor=2, mode="nearest")
    if skip is not None:
        y = torch.cat([y, skip], 1)
    return F.pad(y, (1, 1, 1, 1), mode="reflect")


def _device_inputs(case):
    dev = torch.device("cuda:0")
    x, skip, g = R.make_inputs(case)
    return x, skip, g, torch.from_numpy(x).to(dev), (None if skip is None else torch.from_numpy(skip).to(dev)), torch.from_numpy(g).to(dev)


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_forward_is_bit_equal_to_aten(case):
    from mal_amd.glue import decoder_join
    up, elu, B, C, Cs, h, w = case
    x, skip, g, dx, dskip, dg = _device_inputs(case)
    got = decoder_join(dx, dskip, up=up, elu=bool(elu))
    ref = aten_composition(dx, dskip, up, elu)
    assert got.shape == ref.shape == (B, C + Cs, up * h + 2, up * w + 2)
    assert got.is_contiguous()
    # the sign of zero counts: compare the words
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), float((got - ref).abs().max())
    exact = R.forward(x.astype(np.float64), None if skip is None else skip.astype(np.float64), up, elu)
    print(R.case_id(case), "max |out - fp64|", float(np.abs(got.cpu().numpy().astype(np.float64) - exact).max()))


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_backward_within_the_derived_bound(case):
    from mal_amd.glue import decoder_join, decoder_join_bwd
    up, elu, B, C, Cs, h, w = case
    x, skip, g, dx, dskip, dg = _device_inputs(case)
    lx = dx.clone().requires_grad_(True)
    ls = dskip.clone().requires_grad_(True) if dskip is not None else None
    out = decoder_join(lx, ls, up=up, elu=bool(elu))
    out.backward(dg)
    gx, gskip = lx.grad.cpu().numpy().astype(np.float64), (ls.grad.cpu().numpy().astype(np.float64) if ls is not None else None)
    # exact: fp64 sums, the fp32 factor of the forward's own output
    a = None
    if elu:
        y = out.detach()[:, :C, 1:-1:up, 1:-1:up].cpu().numpy()
        assert y.shape == x.shape
        a = np.where(y > 0, np.float32(1), y + np.float32(1)).astype(np.float32).astype(np.float64)
    g64 = g.astype(np.float64)
    ex, es = R.backward(g64, x.astype(np.float64), up, elu, a=a)
    ax, as_ = R.gathered(np.abs(g64), C, h, w, up)  # sum |terms|
    nx, ns = R.term_counts(h, w, up)
    bound_x = nx[None, None] * U * (np.abs(a) if elu else 1.0) * ax
    bound_s = ns[None, None] * U * as_
    err_x = np.abs(gx - ex)
    print(R.case_id(case), "gx: max err / bound", float((err_x / np.maximum(bound_x, 1e-300)).max()))
    assert (err_x <= bound_x).all()
    if Cs:
        err_s = np.abs(gskip - es)
        print(R.case_id(case), "gskip: max err / bound", float((err_s / np.maximum(bound_s, 1e-300)).max()))
        assert (err_s <= bound_s).all()
    # ATen's own backward on the device
    tx = dx.clone().requires_grad_(True)
    ts = dskip.clone().requires_grad_(True) if dskip is not None else None
    aten_composition(tx, ts, up, elu).backward(dg)
    err = np.abs(tx.grad.cpu().numpy().astype(np.float64) - ex)
    print(R.case_id(case), "ATen gx: max err / bound", float((err / np.maximum(bound_x, 1e-300)).max()))
    assert (err <= 2 * bound_x).all()
    if Cs:
        assert (np.abs(ts.grad.cpu().numpy().astype(np.float64) - es) <= 2 * bound_s).all()
    # a null output leaves the other one as it was
    only_x, none_s = decoder_join_bwd(dg, dx if elu else None, Cs, up, bool(elu), need_x=True, need_skip=False, shape=tuple(dx.shape))
    assert none_s is None and torch.equal(only_x, lx.grad)
    if Cs:
        none_x, only_s = decoder_join_bwd(dg, dx if elu else None, Cs, up, bool(elu), need_x=False, need_skip=True, shape=tuple(dx.shape))
        assert none_x is None and torch.equal(only_s, ls.grad)


def test_only_the_requested_gradients_are_computed():
    from mal_amd.glue import decoder_join
    case = R.CASES[4]
    up, elu, B, C, Cs, h, w = case
    x, skip, g, dx, dskip, dg = _device_inputs(case)
    full_x, full_s = dx.clone().requires_grad_(True), dskip.clone().requires_grad_(True)
    decoder_join(full_x, full_s, up=up, elu=True).backward(dg)
    lx = dx.clone().requires_grad_(True)
    decoder_join(lx, dskip, up=up, elu=True).backward(dg)
    assert torch.equal(lx.grad, full_x.grad)
    ls = dskip.clone().requires_grad_(True)
    decoder_join(dx, ls, up=up, elu=True).backward(dg)
    assert torch.equal(ls.grad, full_s.grad)
    out = decoder_join(lx, None, up=1, elu=False)  # without the activation nothing is saved
    assert out.grad_fn.saved_tensors == ()


def test_replays_from_a_captured_graph():
    from mal_amd.glue import decoder_join
    case = R.CASES[6]  # (2,1,1,5,3,33,70)
    up, elu, B, C, Cs, h, w = case
    x, skip, g, dx, dskip, dg = _device_inputs(case)
    x2, skip2, g2 = R.make_inputs(case, seed=1)
    dev = dx.device
    sx, ss, sg = dx.clone().requires_grad_(True), dskip.clone().requires_grad_(True), dg.clone()
    hold = {}

    def one():
        sx.grad = ss.grad = None
        hold["out"] = decoder_join(sx, ss, up=up, elu=True)
        hold["out"].backward(sg)

    s_ = torch.cuda.Stream()  # eager runs on a side stream first, as tests/test_gpu_step.py captures
    s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        one()
        one()
    torch.cuda.current_stream().wait_stream(s_)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        one()
    out, gx, gs = hold["out"], sx.grad, ss.grad
    for xi, si, gi in ((x2, skip2, g2), (x, skip, g)):
        with torch.no_grad():
            sx.copy_(torch.from_numpy(xi).to(dev))
            ss.copy_(torch.from_numpy(si).to(dev))
            sg.copy_(torch.from_numpy(gi).to(dev))
        out.detach().zero_(), gx.zero_(), gs.zero_()
        graph.replay()
        torch.cuda.synchronize()
        ex = torch.from_numpy(xi).to(dev).requires_grad_(True)
        es = torch.from_numpy(si).to(dev).requires_grad_(True)
        eo = decoder_join(ex, es, up=up, elu=True)
        eo.backward(torch.from_numpy(gi).to(dev))
        assert torch.equal(out.detach(), eo.detach())
        assert torch.equal(gx, ex.grad) and torch.equal(gs, es.grad)


# ------------------------------------------------------------------------------------------------------------ decoder
NUM_CH_ENC = [64, 64, 128, 256, 512]


def _features(B, H, W, seed, dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(B, c, H >> (i + 1), W >> (i + 1), generator=gen, dtype=torch.float64).to(dtype) for i, c in enumerate(NUM_CH_ENC)]


def _run_decoder(dec, feats, cot):
    feats = [f.clone().requires_grad_(True) for f in feats]
    for p in dec.parameters():
        p.grad = None
    disp = dec(feats)[("disp", 0)]
    (disp * cot).sum().backward()
    grads = {"feature_%d" % i: f.grad for i, f in enumerate(feats)}
    grads.update({k: p.grad for k, p in dec.named_parameters()})
    return disp.detach(), grads


def _l2rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def test_fused_decoder_against_the_unfused_one():
    from mal_amd import networks
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    plain = networks.DepthDecoder(NUM_CH_ENC, [0])
    fused = networks.DepthDecoder(NUM_CH_ENC, [0], fused_glue=True)
    fused.load_state_dict(plain.state_dict())
    exact = networks.DepthDecoder(NUM_CH_ENC, [0]).double()
    exact.load_state_dict(plain.state_dict())
    feats = _features(2, 64, 96, seed=5)
    assert tuple(feats[-1].shape[2:]) == (2, 3)
    cot = torch.randn(2, 1, 64, 96, generator=torch.Generator().manual_seed(6))
    ref_disp, ref = _run_decoder(exact, [f.double() for f in feats], cot.double())  # unfused, fp64, CPU
    plain.to(dev), fused.to(dev)
    old = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    # MIOpen's default choice for the two smallest convolutions (2x3 and 4x6 maps) does not reproduce its own output from one
    # call to the next (measured: the unfused decoder differs from itself by one ulp of the disparity); ask for its
    # deterministic solvers, so that equal inputs give equal outputs
    torch.backends.cudnn.deterministic = True
    try:
        d_plain, g_plain = _run_decoder(plain, [f.to(dev) for f in feats], cot.to(dev))
        d_fused, g_fused = _run_decoder(fused, [f.to(dev) for f in feats], cot.to(dev))
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = old
        torch.backends.cudnn.deterministic = det
    print("max |disp fused - disp unfused|", float((d_fused - d_plain).abs().max()))
    assert torch.equal(d_fused, d_plain)  # the convolutions saw bit-identical inputs
    assert set(g_fused) == set(g_plain) == set(ref) and len(ref) == 5 + 22
    for k in sorted(ref):
        own, got = _l2rel(g_plain[k], ref[k]), _l2rel(g_fused[k], ref[k])
        gate = max(1e-4, 1.25 * own)
        print("%-40s unfused %.3e fused %.3e gate %.3e" % (k, own, got, gate))
        assert got <= gate, (k, got, own)


# ------------------------------------------------------------------------------------------------------------ harness
def test_harness_with_the_fused_decoder(tmp_path):
    import random
    from mal_amd import harness
    dev = torch.device("cuda:0")
    kw = dict(batch_size=2, height=96, width=160, no_matching_augmentation=True)
    random.seed(3)
    torch.manual_seed(3)
    plain = harness.TrainHarness(harness.default_options(**kw), dev)
    fused = harness.TrainHarness(harness.default_options(fused_decoder=True, **kw), dev)
    assert fused.model.depth.fused_glue and fused.model.mono_depth.fused_glue
    assert not plain.model.depth.fused_glue and not plain.model.mono_depth.fused_glue
    plain.save(str(tmp_path))
    fused.load(str(tmp_path))  # a checkpoint written without the option loads with it
    for (ka, va), (kb, vb) in zip(plain.model.state_dict().items(), fused.model.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    inputs = harness.synthetic_inputs(fused.opt, dev, seed=7)
    lo, hi = fused.tracker.compute()
    old = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.deterministic = True  # as in the decoder test: equal inputs must give equal convolutions
    try:
        outs = []
        for hz in (plain, fused):
            hz.model.eval()
            with torch.no_grad():
                outs.append(hz.model.val_forward(inputs, lo, hi))
            hz.model.train()
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        for _ in range(2):
            losses = fused.train_step(inputs)
            assert bool(torch.isfinite(losses["loss"]).all()), losses["loss"]
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = old
        torch.backends.cudnn.deterministic = det
