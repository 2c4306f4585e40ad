"""CPU: the restatement of the encoder glue (tests/encoder_glue_cases.py) against torch.autograd of F.batch_norm(...) + r then
relu in fp64 over the shared case table; mal_bn_join_plan (pure host code) covers every element exactly once and its
workspace holds its partials; the argument checks of mal_bn_join_* (no device is touched); and what needs no device of the
Python layer: CPU tensors raise, the fallback predicate, the state dict, the option's default."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import encoder_glue_cases as R


@pytest.fixture(scope="module")
def lib():
    from mal_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_restatement_matches_torch_fp64(lib):
    worst = 0.0
    for case in R.cases():
        (B, C, H, W), mode, mean = case
        if B * C * H * W > 300000:  # the two large shapes add nothing on the CPU that (3,64,6,20) does not
            continue
        x, r, g, gamma, beta, rm, rv = (None if t is None else t.double() for t in R.make_inputs(case))
        relu = R.relu_of(mode)
        leaves = [t.clone().requires_grad_(True) for t in (x, gamma, beta)]
        lr = r.clone().requires_grad_(True) if r is not None else None
        trm, trv = rm.clone(), rv.clone()
        out = F.batch_norm(leaves[0], trm, trv, leaves[1], leaves[2], True, 0.1, R.EPS)
        if lr is not None:
            out = out + lr
        if relu:
            out = F.relu(out)
        out.backward(g)
        N = B * H * W
        m, v = R.statistics(x)
        y, pre, xh = R.forward(x, r, gamma, beta, relu, m, v)
        dx, dr, dgamma, dbeta = R.backward(g, x, gamma, relu, m, v, mask=y > 0)
        erm, erv = R.running(rm, rv, m, v, N, 0.1)
        for got, ref in ((y, out), (dx, leaves[0].grad), (dgamma, leaves[1].grad), (dbeta, leaves[2].grad), (erm, trm), (erv, trv)):
            worst = max(worst, R.l2rel(got, ref))
        if lr is not None:
            worst = max(worst, R.l2rel(dr, lr.grad))
        # N = 2 and a tiny variance: dx cancels to eps/var of its terms, in fp64 too
        assert worst <= 1e-9, (R.case_id(case), worst)
    print("worst L2 rel of the restatement against torch.autograd in fp64: %.2e" % worst)


def test_plan_covers_every_element_once(lib):
    shapes = R.shapes()
    assert len(R.boundary_shapes()) >= 2 and len(R.boundary_shapes()) % 2 == 0
    for lo, hi in zip(R.boundary_shapes()[::2], R.boundary_shapes()[1::2]):
        assert R.plan(*lo)[0] != R.plan(*hi)[0] and hi[0] == lo[0] + 1
    for (B, C, H, W) in shapes + [(12, 64, 96, 320), (12, 64, 48, 160), (12, 128, 24, 80), (12, 256, 12, 40), (12, 512, 6, 20)]:
        S, nbytes = R.plan(B, C, H, W)
        assert 1 <= S <= 64
        assert nbytes >= C * S * 3 * 8  # (n, mean, M2) in fp64 per (channel, block); the backward's two sums fit inside
        for V in ((4, 1) if (H * W) % 4 == 0 else (1,)):  # the 16-byte units and the 4-byte ones
            R_, U = H * W // V, B * (H * W // V)
            upb = -(-U // S)
            seen = torch.zeros(B * H * W, dtype=torch.int32)
            for s in range(S):
                u = torch.arange(s * upb, min((s + 1) * upb, U))
                b, q = u // R_, u % R_
                for k in range(V):
                    seen.index_add_(0, b * (H * W) + q * V + k, torch.ones(len(u), dtype=torch.int32))
            assert bool((seen == 1).all()), (B, C, H, W, V)
    # the stem is split, layer4 is not
    assert R.plan(12, 64, 96, 320)[0] > 1 and R.plan(12, 512, 6, 20)[0] == 1


def test_invalid_arguments_are_refused_without_a_device(lib):
    import ctypes
    p, n, E = 4096, None, -1  # a non-null "pointer" that is never dereferenced: every call below returns before any HIP call
    ok = dict(B=2, C=3, H=4, W=5, eps=1e-5, momentum=0.1, training=1, relu=1, ws=p, ws_bytes=1 << 20)

    def f(x=p, r=p, gamma=p, beta=p, rm=p, rv=p, nbt=p, y=p, sm=p, si=p, **kw):
        a = dict(ok, **kw)
        return lib.mal_bn_join_fwd(x, r, gamma, beta, rm, rv, nbt, y, sm, si, a["B"], a["C"], a["H"], a["W"], a["eps"],
                                   a["momentum"], a["training"], a["relu"], a["ws"], a["ws_bytes"], n)

    def b(g=p, x=p, y=p, gamma=p, sm=p, si=p, dx=p, dr=p, dg=p, db=p, **kw):
        a = dict(ok, **kw)
        return lib.mal_bn_join_bwd(g, x, y, gamma, sm, si, dx, dr, dg, db, a["B"], a["C"], a["H"], a["W"], a["relu"], a["ws"],
                                   a["ws_bytes"], n)

    for name in ("x", "gamma", "beta", "rm", "rv", "nbt", "y", "sm", "si"):
        assert f(**{name: n}) == E, name
    for name in ("g", "x", "y", "gamma", "sm", "si"):
        assert b(**{name: n}) == E, name
    assert f(ws=n) == E and b(ws=n) == E
    assert f(ws_bytes=8) == -3 and b(ws_bytes=8) == -3
    for call in (f, b):
        for bad in (dict(B=0), dict(C=0), dict(H=0), dict(W=0), dict(B=-1), dict(relu=2), dict(relu=-1),
                    dict(B=1, H=1, W=1),                                 # one value per channel
                    dict(B=64, C=512, H=256, W=256),                     # 2^31 elements
                    dict(B=1, C=1, H=2 ** 30, W=2 ** 30), dict(B=2 ** 31 - 1, C=2 ** 31 - 1)):
            assert call(**bad) == E, (call.__name__, bad)
    for bad in (dict(training=2), dict(eps=-1.0), dict(eps=float("inf")), dict(eps=float("nan")), dict(momentum=-0.1),
                dict(momentum=1.5)):
        assert f(**bad) == E, bad
    assert b(dx=n, dr=n, dg=n, db=n) == 0  # nothing to compute: fine, and still no device call
    blocks, nbytes = ctypes.c_int(0), ctypes.c_size_t(0)
    assert lib.mal_bn_join_plan(0, 1, 1, 1, ctypes.byref(blocks), ctypes.byref(nbytes)) == E
    assert lib.mal_bn_join_plan(64, 512, 256, 256, ctypes.byref(blocks), ctypes.byref(nbytes)) == E
    assert lib.mal_bn_join_plan(2, 3, 4, 5, None, None) == 0


def test_cpu_tensors_raise(lib):
    from mal_amd import _lib, networks
    from mal_amd.glue import bn_join
    bn = nn.BatchNorm2d(3)
    with pytest.raises(_lib.MalError):
        bn_join(torch.rand(2, 3, 4, 4), bn)
    with pytest.raises(_lib.MalError):
        bn_join(torch.rand(2, 3, 4, 4), bn, torch.rand(2, 3, 4, 4), relu=False)
    blk = networks.BasicBlock(4, 4, fused_glue=True)
    with pytest.raises(_lib.MalError):
        blk(torch.rand(2, 4, 6, 6))
    enc = networks.ResnetEncoder(18, False, fused_glue=True)
    with pytest.raises(_lib.MalError):
        enc(torch.rand(1, 3, 32, 64))


def test_every_fallback_condition_is_detected():
    from mal_amd.glue import bn_join_fallback_reason as why
    x = torch.rand(2, 3, 4, 4)
    bn = nn.BatchNorm2d(3)
    assert why(x, bn) is None and why(x, bn, torch.rand(2, 3, 4, 4)) is None
    assert "momentum" in why(x, nn.BatchNorm2d(3, momentum=None))
    assert "track_running_stats" in why(x, nn.BatchNorm2d(3, track_running_stats=False))
    assert "affine" in why(x, nn.BatchNorm2d(3, affine=False))
    assert "contiguous" in why(x.to(memory_format=torch.channels_last), bn)
    assert "contiguous" in why(torch.rand(2, 3, 4, 8)[..., ::2], bn)
    assert "float32" in why(x.double(), bn) and "float32" in why(x.half(), bn) and "float32" in why(x.bfloat16(), bn)
    assert "residual" in why(x, bn, torch.rand(2, 3, 4, 4).to(memory_format=torch.channels_last))
    assert "residual" in why(x, bn, torch.rand(2, 3, 4, 5)) and "residual" in why(x, bn, torch.rand(2, 3, 4, 4).double())
    assert "(B,C,H,W)" in why(torch.rand(2, 3, 4), bn)
    # eval mode: the kernels serve it only where nothing asks for a gradient
    ev = nn.BatchNorm2d(3).eval()
    assert "eval" in why(x, ev) and "eval" in why(x.clone().requires_grad_(True), ev)
    with torch.no_grad():
        assert why(x, ev) is None
    for p in ev.parameters():
        p.requires_grad_(False)
    assert why(x, ev) is None and "eval" in why(x.clone().requires_grad_(True), ev)
    assert "eval" in why(x, ev, torch.rand(2, 3, 4, 4).requires_grad_(True))
    # training mode with gradients is the kernels' own ground
    assert why(x.clone().requires_grad_(True), bn) is None


def test_state_dict_and_option_default():
    from mal_amd import harness, networks
    kw = dict(height=32, width=64)
    assert harness.default_options().fused_encoder is False
    assert harness.default_options(fused_encoder=True).fused_encoder is True
    plain = networks.RepDepth(harness.default_options(**kw))
    fused = networks.RepDepth(harness.default_options(fused_encoder=True, **kw))
    a, b = plain.state_dict(), fused.state_dict()
    assert list(a) == list(b)
    assert [(k, tuple(v.shape), v.dtype) for k, v in a.items()] == [(k, tuple(v.shape), v.dtype) for k, v in b.items()]
    assert [n for n, _ in plain.named_modules()] == [n for n, _ in fused.named_modules()]
    blocks = lambda m: [x for x in m.modules() if isinstance(x, networks.BasicBlock)]
    assert len(blocks(fused)) == 24 and all(x.fused_glue for x in blocks(fused)) and not any(x.fused_glue for x in blocks(plain))
    for enc in (fused.encoder, fused.mono_encoder, fused.pose_encoder):
        assert enc.fused_glue is True
    for enc in (plain.encoder, plain.mono_encoder, plain.pose_encoder):
        assert enc.fused_glue is False
    # read at forward time: the switch of an encoder reaches its blocks, and back
    plain.encoder.fused_glue = True
    assert all(x.fused_glue for x in blocks(plain.encoder)) and not any(x.fused_glue for x in blocks(plain.mono_encoder))
    plain.encoder.fused_glue = False
    assert not any(x.fused_glue for x in blocks(plain))
    fused.load_state_dict(a, strict=True)
    plain.load_state_dict(b, strict=True)
