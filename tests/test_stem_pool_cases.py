"""CPU: the restatement of the stem max-pool (tests/stem_pool_restated.py) against torch's own max_pool2d on the CPU over the
shared case table -- values, indices and the gradient routing; torch is the arbiter of the tie rule --; the proof that the tie
fillings tell the first of equal maxima from the last; mal_stem_pool_plan (pure host code) and the argument checks of
mal_stem_pool_* (no device is touched); and what needs no device of the Python layer: CPU tensors raise, the fallback
predicate, the state dict, the option's default."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import stem_pool_cases as T
from tests import stem_pool_restated as R


@pytest.fixture(scope="module")
def lib():
    from mal_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def _torch_pool(y):
    return F.max_pool2d(y, kernel_size=3, stride=2, padding=1, return_indices=True)


@pytest.mark.parametrize("shape", T.SHAPES + list(T.STRIDED.values()), ids=lambda s: "x".join(map(str, s)))
def test_restatement_matches_torch(shape):
    fillings = T.STRIDED_FILLINGS if shape in T.STRIDED.values() else T.FILLINGS
    for filling in fillings:
        case = (shape, filling)
        y = T.make_input(case)
        p, code, index = R.forward(y)
        tp, ti = _torch_pool(torch.from_numpy(y.copy()))
        assert p.dtype == np.float32 and code.dtype == np.uint8
        assert np.array_equal(p, tp.numpy(), equal_nan=True), T.case_id(case)
        assert np.array_equal(np.isnan(p), torch.isnan(tp).numpy()), T.case_id(case)
        assert np.array_equal(index, ti.numpy()), T.case_id(case)
        assert code.min() >= 0 and code.max() <= 8
        # any dtype: the fp64 restatement picks the same winners
        assert np.array_equal(R.forward(y.astype(np.float64))[1], code)
        # the gradient routing: torch.autograd through max_pool2d plus the skip term, in fp64
        for integer in (False, True):
            g_p, g_y = T.make_cotangents(case, integer)
            leaf = torch.from_numpy(y.astype(np.float64)).requires_grad_(True)
            (grad,) = torch.autograd.grad([_torch_pool(leaf)[0], leaf * 1.0], [leaf],
                                          [torch.from_numpy(g_p.astype(np.float64)), torch.from_numpy(g_y.astype(np.float64))])
            dy = R.backward(g_p, g_y, code, shape)
            assert dy.dtype == np.float64 and dy.shape == tuple(shape)
            if integer:
                assert np.array_equal(dy, grad.numpy()), T.case_id(case)
            else:
                assert np.allclose(dy, grad.numpy(), rtol=1e-13, atol=1e-13), T.case_id(case)
            (alone,) = torch.autograd.grad(_torch_pool(leaf)[0], leaf, torch.from_numpy(g_p.astype(np.float64)))
            assert np.allclose(R.backward(g_p, None, code, shape), alone.numpy(), rtol=1e-13, atol=1e-13)
            # every cotangent arrives exactly once
            if integer:
                assert R.backward(g_p, None, code, shape).sum() == g_p.astype(np.float64).sum()


def test_the_tie_fillings_tell_first_max_from_last_max():
    """the restatement with the comparison turned to >= (the last of equal maxima) must fail the tie fillings"""
    for filling in ("zeros", "threes"):
        for shape in T.SHAPES:
            y = T.make_input((shape, filling))
            ti = _torch_pool(torch.from_numpy(y.copy()))[1].numpy()
            assert np.array_equal(R.forward(y)[2], ti)
            if shape[2] * shape[3] > 1:  # a window of two elements or more
                assert not np.array_equal(R.forward(y, ge=True)[2], ti), (shape, filling)
    for filling in ("relu", "integers"):
        for shape in [(3, 64, 6, 20), (2, 3, 5, 7)] + T.WIDTH_SHAPES:
            y = T.make_input((shape, filling))
            ti = _torch_pool(torch.from_numpy(y.copy()))[1].numpy()
            wrong = R.forward(y, ge=True)
            assert np.array_equal(wrong[0], R.forward(y)[0])  # the same values: only the indices show it
            assert not np.array_equal(wrong[2], ti), (shape, filling)
    # and a plane of -inf keeps the window's first element under torch's rule only
    y = T.make_input(((2, 3, 5, 7), "neg_inf_plane"))
    ti = _torch_pool(torch.from_numpy(y.copy()))[1].numpy()
    assert np.array_equal(R.forward(y)[2], ti) and not np.array_equal(R.forward(y, ge=True)[2], ti)
    # two NaNs in one window: the later one wins it
    y = T.make_input(((2, 3, 5, 7), "nan_pair"))
    assert (R.forward(y)[1][:, :, 0, 0] == 8).all() and (R.forward(y)[2][:, :, 0, 0] == 1 * 7 + 1).all()


def test_plan_arithmetic(lib):
    threads, cap = 256, 2048
    for shape in T.SHAPES + list(T.STRIDED.values()) + [(12, 64, 96, 320), (24, 64, 96, 320), (12, 64, 97, 322)]:
        B, C, H, W = shape
        for aligned in (True, False):
            OH, OW, bf, bb, vf, vb = T.plan(shape, aligned)
            assert (OH, OW) == T.out_shape(shape)[2:]
            assert vf == (4 if aligned and W % 8 == 0 else 1) and vb == (4 if aligned and W % 4 == 0 else 1)
            uf, ub = B * C * OH * (OW // vf), B * C * H * (W // vb)
            assert OW % vf == 0 and W % vb == 0  # a thread's unit never crosses a row's end
            assert bf == min(-(-uf // threads), cap) and bb == min(-(-ub // threads), cap)
            assert 1 <= bf <= cap and 1 <= bb <= cap
    # the two strided shapes pass over the grid more than once on the routes they are named for; the table's own never do
    assert all(n > 1 for n in T.sweeps(T.STRIDED["one_float_routes"], aligned=True))       # odd W: one float whatever the pointers
    assert T.plan(T.STRIDED["one_float_routes"])[4:] == (1, 1)
    assert all(n > 1 for n in T.sweeps(T.STRIDED["sixteen_byte_routes"], aligned=True))
    assert T.plan(T.STRIDED["sixteen_byte_routes"])[4:] == (4, 4)
    assert all(T.sweeps(s, a) == (1, 1) for s in T.SHAPES for a in (True, False))
    # the training shape: three sweeps forward, twelve backward
    assert T.sweeps((12, 64, 96, 320)) == (3, 12)


def test_invalid_arguments_are_refused_without_a_device(lib):
    p, n, E = 4096, None, -1  # a non-null "pointer" that is never dereferenced: every call below returns before any HIP call
    ok = dict(B=2, C=3, H=4, W=5)
    bad_shapes = (dict(B=0), dict(C=0), dict(H=0), dict(W=0), dict(B=-1), dict(W=-3),
                  dict(B=64, C=512, H=256, W=256),                     # 2^31 elements
                  dict(B=1, C=1, H=2 ** 30, W=2 ** 30), dict(B=2 ** 31 - 1, C=2 ** 31 - 1))

    def f(y=p, out=p, code=p, **kw):
        a = dict(ok, **kw)
        return lib.mal_stem_pool_fwd(y, out, code, a["B"], a["C"], a["H"], a["W"], n)

    def b(g_p=p, g_y=p, code=p, dy=p, **kw):
        a = dict(ok, **kw)
        return lib.mal_stem_pool_bwd(g_p, g_y, code, dy, a["B"], a["C"], a["H"], a["W"], n)

    def plan(**kw):
        a = dict(ok, **kw)
        outs = [ctypes.c_int(0) for _ in range(6)]
        return lib.mal_stem_pool_plan(a["B"], a["C"], a["H"], a["W"], 1, *[ctypes.byref(o) for o in outs])

    assert f(y=n) == E and f(out=n) == E
    for name in ("g_p", "code", "dy"):
        assert b(**{name: n}) == E, name
    for call in (f, b, plan):
        for bad in bad_shapes:
            assert call(**bad) == E, (call.__name__, bad)
    assert plan() == 0
    assert lib.mal_stem_pool_plan(2, 3, 4, 5, 1, None, None, None, None, None, None) == 0
    assert lib.mal_stem_pool_plan(32, 512, 256, 511, 1, None, None, None, None, None, None) == 0  # just below 2^31


def test_cpu_tensors_raise(lib):
    from mal_amd import _lib, networks
    from mal_amd.glue import stem_pool, stem_pool_fwd
    with pytest.raises(_lib.MalError):
        stem_pool(torch.rand(2, 3, 4, 4))
    with pytest.raises(_lib.MalError):
        stem_pool(torch.rand(2, 3, 4, 4), nn.MaxPool2d(3, 2, 1))
    with pytest.raises(_lib.MalError):
        stem_pool(torch.rand(2, 3, 4, 4), nn.MaxPool2d(2))  # also where the kernels would not apply
    with pytest.raises(_lib.MalError):
        stem_pool_fwd(torch.rand(2, 3, 4, 4))
    for enc in (networks.ResnetEncoder(18, False, fused_pool=True), networks.ResNet18(fused_pool=True)):
        with pytest.raises(_lib.MalError):
            enc(torch.rand(1, 3, 32, 64))
    enc = networks.ResnetEncoderMatching(18, False, 32, 64, fused_pool=True)
    with pytest.raises(_lib.MalError):
        enc.feature_extraction(torch.rand(1, 3, 32, 64))
    # off, the same modules run on the CPU as they always did
    assert networks.ResnetEncoder(18, False)(torch.rand(1, 3, 32, 64))[1].shape == (1, 64, 8, 16)
    assert networks.ResNet18()(torch.rand(1, 3, 32, 64)).shape == (1, 1000)


def test_every_fallback_condition_is_detected():
    from mal_amd.glue import stem_pool_fallback_reason as why
    y = torch.rand(2, 3, 6, 8)
    good = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
    assert why(y, good) is None and why(y) is None
    assert why(y, nn.MaxPool2d((3, 3), (2, 2), (1, 1), (1, 1))) is None
    assert why(y.clone().requires_grad_(True), good) is None
    # every non-default argument of the module
    assert "kernel_size" in why(y, nn.MaxPool2d(2, 2, 1)) and "kernel_size" in why(y, nn.MaxPool2d((3, 2), 2, 1))
    assert "kernel_size" in why(y, nn.MaxPool2d(2))
    assert "stride" in why(y, nn.MaxPool2d(3, 1, 1)) and "stride" in why(y, nn.MaxPool2d(3, (2, 1), 1))
    assert "stride" in why(y, nn.MaxPool2d(3, padding=1))  # stride defaults to the kernel size
    assert "padding" in why(y, nn.MaxPool2d(3, 2, 0)) and "padding" in why(y, nn.MaxPool2d(3, 2, (1, 0)))
    assert "dilation" in why(y, nn.MaxPool2d(3, 2, 1, dilation=2)) and "dilation" in why(y, nn.MaxPool2d(3, 2, 1, dilation=(1, 2)))
    assert "ceil_mode" in why(y, nn.MaxPool2d(3, 2, 1, ceil_mode=True))
    assert "return_indices" in why(y, nn.MaxPool2d(3, 2, 1, return_indices=True))
    assert "MaxPool2d" in why(y, nn.AvgPool2d(3, 2, 1))
    # the tensor
    for dt in (torch.float64, torch.float16, torch.bfloat16):
        assert "float32" in why(y.to(dt), good)
    assert "contiguous" in why(y.to(memory_format=torch.channels_last), good)
    assert "contiguous" in why(torch.rand(2, 3, 6, 16)[..., ::2], good)
    assert "(B,C,H,W)" in why(torch.rand(3, 6, 8), good)
    assert "2^31" in why(torch.empty((2, 2 ** 10, 2 ** 10, 2 ** 10), device="meta"), good)  # no storage behind it
    assert why(torch.empty((2, 2 ** 10, 2 ** 10, 2 ** 9), device="meta"), good) is None


def test_state_dict_and_option_default():
    from mal_amd import harness, networks
    kw = dict(height=32, width=64)
    assert harness.default_options().fused_pool is False
    assert harness.default_options(fused_pool=True).fused_pool is True
    assert harness.default_options(fused_pool=True).fused_encoder is False  # independent switches
    plain = networks.RepDepth(harness.default_options(**kw))
    fused = networks.RepDepth(harness.default_options(fused_pool=True, **kw))
    a, b = plain.state_dict(), fused.state_dict()
    assert list(a) == list(b)
    assert [(k, tuple(v.shape), v.dtype) for k, v in a.items()] == [(k, tuple(v.shape), v.dtype) for k, v in b.items()]
    assert [n for n, _ in plain.named_modules()] == [n for n, _ in fused.named_modules()]
    for enc in (fused.encoder, fused.mono_encoder, fused.pose_encoder):
        assert enc.fused_pool is True and enc.fused_glue is False
    for enc in (plain.encoder, plain.mono_encoder, plain.pose_encoder):
        assert enc.fused_pool is False
    both = networks.RepDepth(harness.default_options(fused_pool=True, fused_encoder=True, **kw))
    assert all(e.fused_pool and e.fused_glue for e in (both.encoder, both.mono_encoder, both.pose_encoder))
    assert isinstance(fused.encoder.layer1[0], nn.MaxPool2d) and isinstance(fused.mono_encoder.encoder.maxpool, nn.MaxPool2d)
    fused.load_state_dict(a, strict=True)
    plain.load_state_dict(b, strict=True)
