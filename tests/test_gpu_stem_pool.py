"""GPU: mal_amd.glue.stem_pool (mal_amd/csrc/mal_pool.hip) over the case table of tests/stem_pool_cases.py, the three encoders with
``fused_pool`` set against their unfused copies, and the harness with the option set.

Truth is the numpy restatement (tests/test_stem_pool_cases.py holds it to torch on the CPU) and torch's own max_pool2d on the
device.  Selection is exact: values bit for bit, codes equal to torch's indices everywhere, no near-tie allowance.  The backward
is a sum of at most five fp32 terms in a fixed order: |dy - exact| <= 4 * 2^-24 * (|g_y| + sum |g_p terms|) per element (four
roundings) against the fp64 restatement, and equal to the ATen route exactly where the cotangents are small integers.
Each case is evaluated once (evaluate(): every figure of the tests below) and the tests read the record."""
import copy
import functools
import random

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import stem_pool_cases as T
from tests import stem_pool_restated as R

pytestmark = pytest.mark.gpu
CASES = T.cases()
IDS = [T.case_id(c) for c in CASES]
BOUND = 4.0 * 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


def dev():
    return torch.device("cuda:0")


def same_words(a, b):
    """bit for bit (a NaN equals the same NaN, +0 does not equal -0)"""
    a, b = a.detach().contiguous(), b.detach().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _aten(y):
    return F.max_pool2d(y, kernel_size=3, stride=2, padding=1)


def _fused_grad(y, g_p, g_y):
    """dy through autograd: the cotangents of (the returned y, p), either may be None"""
    from mal_amd.glue import stem_pool
    leaf = y.clone().requires_grad_(True)
    out_y, p = stem_pool(leaf)
    outs, gs = ([p], [g_p]) if g_y is None else (([out_y], [g_y]) if g_p is None else ([out_y, p], [g_y, g_p]))
    return torch.autograd.grad(outs, [leaf], gs)[0]


def _aten_grad(y, g_p, g_y):
    """the ATen route: max_pool2d's backward plus autograd's accumulation with the skip's cotangent"""
    leaf = y.clone().requires_grad_(True)
    outs, gs = [_aten(leaf)], [g_p]
    if g_y is not None:
        outs, gs = outs + [leaf.view_as(leaf)], gs + [g_y]
    return torch.autograd.grad(outs, [leaf], gs)[0]


@functools.lru_cache(None)
def evaluate(case):
    from mal_amd.glue import stem_pool, stem_pool_fallback_reason
    shape, filling = case
    B, C, H, W = shape
    y_np = T.make_input(case)
    p_ref, code_ref, index_ref = R.forward(y_np)
    y = _to(y_np)
    rec = {"fallback": stem_pool_fallback_reason(y, nn.MaxPool2d(3, 2, 1))}
    # ---- forward with a graph
    leaf = y.clone().requires_grad_(True)
    out_y, p = stem_pool(leaf)
    (code,) = p.grad_fn.saved_tensors
    rec["node"] = p.grad_fn is out_y.grad_fn and p.grad_fn is not None and out_y.data_ptr() == leaf.data_ptr()
    rec["saved"] = (len(p.grad_fn.saved_tensors), code.dtype, tuple(code.shape))
    rec["p_bits"] = same_words(p, _to(p_ref))
    rec["nan_positions"] = np.array_equal(np.isnan(p.detach().cpu().numpy()), np.isnan(p_ref))
    code_np = code.cpu().numpy()
    rec["code_restated"] = np.array_equal(code_np, code_ref)
    ap, ai = F.max_pool2d(y, kernel_size=3, stride=2, padding=1, return_indices=True)
    rec["code_torch"] = bool(code_np.max() <= 8) and np.array_equal(R.index_of(code_np, H, W), ai.cpu().numpy())
    rec["p_torch"] = same_words(p, ap)
    # ---- without a graph
    with torch.no_grad():
        ny, np_ = stem_pool(leaf)
    rec["no_grad"] = np_.grad_fn is None and ny is leaf and same_words(np_, p)
    ry, rp = stem_pool(y)  # grad mode on, nothing requires a gradient
    rec["no_leaf"] = rp.grad_fn is None and ry is y and same_words(rp, p)
    # ---- backward
    for integer in (False, True):
        g_p_np, g_y_np = T.make_cotangents(case, integer)
        g_p, g_y = _to(g_p_np), _to(g_y_np)
        tag = "int" if integer else "rnd"
        for with_y in (True, False):
            gy = g_y if with_y else None
            dy = _fused_grad(y, g_p, gy)
            again = _fused_grad(y, g_p, gy)
            key = tag + ("+gy" if with_y else "")
            rec["deterministic_" + key] = same_words(dy, again)
            exact = R.backward(g_p_np, g_y_np if with_y else None, code_ref, shape)
            room = R.backward(np.abs(g_p_np), np.abs(g_y_np) if with_y else None, code_ref, shape)
            err = np.abs(dy.cpu().numpy().astype(np.float64) - exact)
            rec["bound_" + key] = float((err / np.maximum(room * BOUND, 1e-300)).max()) if err.max() > 0 else 0.0
            if integer:
                rec["aten_" + key] = torch.equal(dy, _aten_grad(y, g_p, gy))
                rec["exact_" + key] = np.array_equal(dy.cpu().numpy().astype(np.float64), exact)
        rec["gp_none_" + tag] = torch.equal(_fused_grad(y, None, g_y), g_y)
    return rec


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_is_the_restatement_bit_for_bit(case):
    rec = evaluate(case)
    assert rec["fallback"] is None
    assert rec["p_bits"] and rec["nan_positions"] and rec["p_torch"]
    assert rec["node"] and rec["saved"] == (1, torch.uint8, T.out_shape(case[0]))  # the codes are all the node saves


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_codes_are_torchs_indices(case):
    rec = evaluate(case)
    assert rec["code_torch"] and rec["code_restated"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_bound(case):
    rec = evaluate(case)
    worst = max(rec[k] for k in rec if k.startswith("bound_"))
    print(T.case_id(case), "worst |dy - exact| / (4 * 2^-24 * sum |terms|): %.3f" % worst)
    assert worst <= 1.0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_exact_with_integer_cotangents(case):
    rec = evaluate(case)
    assert rec["aten_int+gy"] and rec["exact_int+gy"]
    assert rec["aten_int"] and rec["exact_int"]  # g_y = None: the pool's gradient alone


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_missing_cotangents_and_determinism(case):
    rec = evaluate(case)
    assert rec["gp_none_rnd"] and rec["gp_none_int"]
    assert all(v for k, v in rec.items() if k.startswith("deterministic_"))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_grad_route(case):
    rec = evaluate(case)
    assert rec["no_grad"] and rec["no_leaf"]


def test_without_the_pools_cotangent_nothing_is_launched(monkeypatch):
    from mal_amd import glue
    g_y = torch.randn(2, 3, 6, 8, device=dev())
    code = torch.zeros(2, 3, 3, 4, dtype=torch.uint8, device=dev())

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)

    monkeypatch.setattr(glue.L, "load", lambda: NoLaunch())
    assert glue.stem_pool_bwd(None, g_y, code, (2, 3, 6, 8)) is g_y
    assert glue.stem_pool_bwd(None, None, code, (2, 3, 6, 8)) is None


def test_no_code_tensor_under_no_grad(monkeypatch):
    from mal_amd import glue
    seen = []
    real = glue.stem_pool_fwd
    monkeypatch.setattr(glue, "stem_pool_fwd", lambda y, need_code=True: seen.append(need_code) or real(y, need_code))
    y = torch.randn(2, 3, 6, 8, device=dev())
    with torch.no_grad():
        glue.stem_pool(y.clone().requires_grad_(True))
    glue.stem_pool(y)
    glue.stem_pool(y.clone().requires_grad_(True))
    assert seen == [False, False, True]
    assert real(y, need_code=False)[1] is None


# ------------------------------------------------------------------------------------- the one-float routes by address
PATTERN = 0x7FC0BEEF  # as a float: a NaN no kernel produces
GUARD = 64


def _window(n, offset, dtype=torch.float32, fill=None):
    """a contiguous run of n elements that starts ``offset`` elements into a buffer prefilled with a bit pattern, GUARD
    elements of it on either side -> (buffer, view)"""
    buf = torch.empty(GUARD + offset + n + GUARD, dtype=dtype, device=dev())
    assert buf.data_ptr() % 16 == 0
    if dtype == torch.float32:
        buf.view(torch.int32).fill_(PATTERN)
    else:
        buf.fill_(0xA5)
    view = buf[GUARD + offset:GUARD + offset + n]
    if fill is not None:
        view.copy_(fill.reshape(-1))
    return buf, view


def _guards_intact(buf, offset, n):
    pat = PATTERN if buf.dtype == torch.float32 else 0xA5
    words = buf.view(torch.int32) if buf.dtype == torch.float32 else buf
    return bool((words[:GUARD + offset] == pat).all()) and bool((words[GUARD + offset + n:] == pat).all())


ROUTE_SHAPES = [(1, 2, 4, 4), (2, 1, 6, 8), (3, 64, 6, 20), (1, 2, 3, 64), (1, 2, 4, 128), (1, 2, 3, 256), (1, 2, 4, 256),
                T.STRIDED["sixteen_byte_routes"]]


@pytest.mark.parametrize("shape", ROUTE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_sixteen_byte_and_the_one_float_routes_give_the_same_bits(shape):
    """through the C entry points: y, p, g_p, g_y and dy held 1, 2 and 3 floats (the codes 1 byte) into larger buffers take
    the one-float routes by address alone; the windows hold the aligned call's bits and the guard words keep their pattern"""
    from mal_amd import _lib as L
    from mal_amd.glue import stem_pool_fwd, stem_pool_bwd
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    B, C, H, W = shape
    case = (shape, "relu")
    assert T.plan(shape, True)[5] == 4 and T.plan(shape, False)[4:] == (1, 1)
    y = _to(T.make_input(case))
    g_p, g_y = (_to(a) for a in T.make_cotangents(case, False))
    p, code = stem_pool_fwd(y)
    dy = stem_pool_bwd(g_p, g_y, code, shape)
    dy_alone = stem_pool_bwd(g_p, None, code, shape)
    n_out, n_in = p.numel(), y.numel()
    for off_y, off_p, off_c in ((1, 0, 0), (0, 2, 0), (0, 0, 1), (1, 2, 3)):
        by, vy = _window(n_in, off_y, fill=y)
        bp, vp = _window(n_out, off_p)
        bc, vc = _window(n_out, off_c, torch.uint8)
        L.check(lib.mal_stem_pool_fwd(vy.data_ptr(), vp.data_ptr(), vc.data_ptr(), B, C, H, W, st), "fwd")
        torch.cuda.synchronize()
        assert same_words(vp.view(p.shape), p) and torch.equal(vc.view(code.shape), code), (off_y, off_p, off_c)
        assert _guards_intact(bp, off_p, n_out) and _guards_intact(bc, off_c, n_out) and _guards_intact(by, off_y, n_in)
    for off_gp, off_gy, off_dy, off_c in ((1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1), (1, 2, 3, 0), (1, 2, 3, 3)):
        bgp, vgp = _window(n_out, off_gp, fill=g_p)
        bgy, vgy = _window(n_in, off_gy, fill=g_y)
        bdy, vdy = _window(n_in, off_dy)
        bc, vc = _window(n_out, off_c, torch.uint8, fill=code)
        for gy_ptr, want in ((vgy.data_ptr(), dy), (None, dy_alone)):
            L.check(lib.mal_stem_pool_bwd(vgp.data_ptr(), gy_ptr, vc.data_ptr(), vdy.data_ptr(), B, C, H, W, st), "bwd")
            torch.cuda.synchronize()
            assert same_words(vdy.view(dy.shape), want), (off_gp, off_gy, off_dy, off_c, gy_ptr is None)
            assert _guards_intact(bdy, off_dy, n_in)
    # and through the Python layer: a view at storage offset 1 is contiguous, takes the one-float route, and no fallback
    from mal_amd.glue import stem_pool, stem_pool_fallback_reason
    _, vy = _window(n_in, 1, fill=y)
    vy = vy.view(shape)
    assert stem_pool_fallback_reason(vy, nn.MaxPool2d(3, 2, 1)) is None and vy.data_ptr() % 16 == 4
    assert same_words(stem_pool(vy)[1], p)


# ------------------------------------------------------------------------------------------------------- graph capture
def test_graph_capture_and_replay():
    from mal_amd.glue import stem_pool
    shape = (3, 64, 6, 20)
    sets = [(_to(T.make_input((shape, f))),) + tuple(_to(a) for a in T.make_cotangents((shape, f), False))
            for f in ("relu", "integers", "normal")]
    sy = sets[0][0].clone().requires_grad_(True)
    sgp, sgy = sets[0][1].clone(), sets[0][2].clone()
    hold = {}

    def one():
        out_y, p = stem_pool(sy)
        hold["p"] = p
        hold["dy"] = torch.autograd.grad([out_y, p], [sy], [sgy, sgp])[0]

    side = torch.cuda.Stream()  # eager runs on a side stream first, as tests/test_gpu_decoder_glue.py captures
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one()
        one()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        one()
    torch.cuda.synchronize()
    outs = (hold["p"], hold["dy"])
    for k, (yi, gpi, gyi) in enumerate(sets[1:], 1):
        with torch.no_grad():
            sy.copy_(yi), sgp.copy_(gpi), sgy.copy_(gyi)
            for t in outs:
                t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        leaf = yi.clone().requires_grad_(True)
        ey, ep = stem_pool(leaf)
        edy = torch.autograd.grad([ey, ep], [leaf], [gyi, gpi])[0]
        assert same_words(outs[0], ep) and same_words(outs[1], edy), k


# ------------------------------------------------------------------------------------------------------------ refusals
def test_cpu_tensors_raise_and_other_pools_fall_back():
    from mal_amd import _lib
    from mal_amd.glue import stem_pool, stem_pool_fallback_reason
    with pytest.raises(_lib.MalError):
        stem_pool(torch.rand(2, 3, 4, 4), nn.MaxPool2d(3, 2, 1))
    y = torch.randn(2, 3, 6, 8, device=dev())
    for pool, yin in ((nn.MaxPool2d(2), y), (nn.MaxPool2d(3, 2, 1, ceil_mode=True), y), (nn.MaxPool2d(3, 2, 1), y.double()),
                      (nn.MaxPool2d(3, 2, 1), y.to(memory_format=torch.channels_last))):
        assert stem_pool_fallback_reason(yin, pool) is not None
        leaf, ref = yin.clone().requires_grad_(True), yin.clone().requires_grad_(True)
        out_y, got = stem_pool(leaf, pool)
        want = pool(ref)
        assert out_y is leaf and torch.equal(got, want)
        g = torch.randn_like(want)
        assert torch.equal(torch.autograd.grad(got, leaf, g)[0], torch.autograd.grad(want, ref, g)[0])
    # return_indices: the module's own tuple comes back
    out_y, (v, i) = stem_pool(y, nn.MaxPool2d(3, 2, 1, return_indices=True))
    rv, ri = F.max_pool2d(y, 3, 2, 1, return_indices=True)
    assert torch.equal(v, rv) and torch.equal(i, ri)


# ------------------------------------------------------------------------------------------------------------ networks
class _Deterministic:
    """MIOpen's deterministic solvers and no TF32: equal inputs give equal convolutions (tests/test_gpu_encoder_glue.py)"""

    def __enter__(self):
        self.old = (torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.deterministic)
        torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
        torch.backends.cudnn.deterministic = True

    def __exit__(self, *exc):
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.deterministic = self.old


def _fixed_cost_volume(cur, look, poses, K, invK, bins, set_missing_to_max=True):
    """stands in for the cost volume (not under test; it has no fp64 CPU form): the same fixed maps for every copy of the model"""
    B, _, h, w = cur.shape
    gen = torch.Generator().manual_seed(17)
    cv = torch.rand(B, len(bins), h, w, generator=gen, dtype=torch.float64).to(cur)
    low = torch.rand(B, h, w, generator=gen, dtype=torch.float64).to(cur)
    return cv, low, (low > 0.5).to(cur)


def _image(B, C, H, W, seed, dt, where):
    return torch.rand(B, C, H, W, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dt).to(where)


def l2rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def _call_encoder(model, dt, where):
    x = _image(2, 3, 32, 64, 4, dt, where).requires_grad_(True)
    return x, list(model(x))


def _call_matching(model, dt, where):
    cur = _image(2, 3, 32, 64, 4, dt, where).requires_grad_(True)
    look = _image(2, 3, 32, 64, 6, dt, where).view(2, 1, 3, 32, 64)
    eye = torch.eye(4, dtype=dt, device=where).expand(2, 4, 4)
    feats, low, conf = model(cur, look, eye.unsqueeze(1), eye, eye, min_depth_bin=0.1, max_depth_bin=20.0)
    return cur, list(feats)  # the pool ran twice: the current image, then the lookup frame without a graph


def _call_resnet(model, dt, where):
    x = _image(2, 3, 32, 64, 4, dt, where).requires_grad_(True)
    return x, [model(x)]


def _models():
    from mal_amd import networks
    return {"ResnetEncoder": (lambda: networks.ResnetEncoder(18, False), _call_encoder),
            "ResnetEncoderMatching": (lambda: networks.ResnetEncoderMatching(18, False, 32, 64, adaptive_bins=True, num_depth_bins=8),
                                      _call_matching),
            "ResNet18": (lambda: networks.ResNet18(num_classes=10), _call_resnet)}


def _run_model(model, call, dt, where):
    """one training-mode forward and backward -> (outputs, {name: gradient})"""
    model.train()
    x, outs = call(model, dt, where)
    gen = torch.Generator().manual_seed(9)
    loss = sum((o * torch.randn(o.shape, generator=gen, dtype=torch.float64).to(o)).sum() for o in outs)
    loss.backward()
    grads = {"grad:" + k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    grads["grad:input"] = x.grad
    return [o.detach() for o in outs], grads


@pytest.mark.parametrize("name", ["ResnetEncoder", "ResnetEncoderMatching", "ResNet18"])
def test_encoders(name, monkeypatch):
    """fused_pool on and off from the same weights, crossed with fused_glue: the features are bit-equal, and the gradients of
    the fused-pool copy lie no further from the same model in fp64 on the CPU than 1.25 x the unfused copy's own distance"""
    from mal_amd import networks
    monkeypatch.setattr(networks.costvol, "cost_volume_outputs", _fixed_cost_volume)
    make, call = _models()[name]
    torch.manual_seed(5)
    exact = make().double()
    for m in exact.modules():  # norms that do something (tests/test_gpu_encoder_glue.py)
        if isinstance(m, nn.BatchNorm2d):
            with torch.no_grad():
                m.weight.uniform_(0.5, 1.5), m.bias.uniform_(-0.3, 0.3)
    with _Deterministic():
        _, ref = _run_model(exact, call, torch.float64, "cpu")
        for glue_on in (False, True):
            res = {}
            for pool_on in (False, True):
                model = make().float()
                model.load_state_dict(exact.state_dict())
                model.to(dev())
                model.fused_glue, model.fused_pool = glue_on, pool_on
                res[pool_on] = _run_model(model, call, torch.float32, dev())
            (outs_off, grads_off), (outs_on, grads_on) = res[False], res[True]
            assert len(outs_on) == len(outs_off)
            for i, (a, b) in enumerate(zip(outs_on, outs_off)):
                assert same_words(a, b), (name, glue_on, "feature %d" % i)
            assert set(grads_on) == set(grads_off) == set(ref)
            for k in sorted(ref):
                own, got = l2rel(grads_off[k], ref[k]), l2rel(grads_on[k], ref[k])
                print("%-22s fused_glue=%d %-44s unfused pool %.3e fused pool %.3e" % (name, glue_on, k, own, got))
                assert got <= 1.25 * own, (name, glue_on, k, got, own)


# ------------------------------------------------------------------------------------------------------------ harness
def test_harness_with_the_fused_pool(tmp_path):
    from mal_amd import harness
    kw = dict(batch_size=2, height=96, width=160, no_matching_augmentation=True)
    random.seed(3)
    torch.manual_seed(3)
    plain = harness.TrainHarness(harness.default_options(**kw), dev())
    fused = harness.TrainHarness(harness.default_options(fused_pool=True, **kw), dev())
    for enc in (fused.model.encoder, fused.model.mono_encoder, fused.model.pose_encoder):
        assert enc.fused_pool and not enc.fused_glue
    for enc in (plain.model.encoder, plain.model.mono_encoder, plain.model.pose_encoder):
        assert not enc.fused_pool
    inputs = harness.synthetic_inputs(fused.opt, dev(), seed=7)
    with _Deterministic():
        for _ in range(2):
            losses = fused.train_step(copy.copy(inputs))
            assert bool(torch.isfinite(losses["loss"]).all()), losses["loss"]
    (tmp_path / "a").mkdir()
    fused.save(str(tmp_path / "a"))
    plain.model.load_state_dict(torch.load(str(tmp_path / "a" / "model.pth"), map_location="cpu"), strict=True)
    plain.load(str(tmp_path / "a"))  # a checkpoint written with the option loads without it
    for (ka, va), (kb, vb) in zip(fused.model.state_dict().items(), plain.model.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    with _Deterministic():  # the next forward, from the same state: the networks' outputs bit for bit
        out_f, _ = fused.process_batch(copy.copy(inputs))
        out_p, _ = plain.process_batch(copy.copy(inputs))
    for key in (("disp", 0), ("mono_disp", 0), "lowest_cost"):
        assert same_words(out_f[key], out_p[key]), key
