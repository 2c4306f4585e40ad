"""GPU: mal_amd.glue.bn_join (mal_amd/csrc/mal_bn.hip) over the case table of tests/encoder_glue_cases.py, the ResNet blocks and
encoders with ``fused_glue`` set against their unfused copies, and the harness with ``fused_encoder`` set.

Truth is the fp64 restatement on the CPU (tests/test_encoder_glue_cases.py holds it to torch.autograd in fp64); the yardstick is
the fp32 ATen composition relu(bn(x) + r) on the same device and inputs.  Gates (L2 rel unless said otherwise):
  y                        max(1e-6, 2 x ATen's distance from fp64)      two legitimate summation orders
  batch variance           relative error <= 1e-5 per channel            between PyTorch's 6e-8 and the naive formula's 2.5e-4;
                           a constant channel (fp64 variance exactly 0) must stay below 1e-5 * eps, the only place it enters
  running statistics       running_var as the variance, running_mean 1e-5 L2 rel, num_batches_tracked exact
  dx, dr, dgamma, dbeta    max(1e-4, 1.25 x ATen's distance), decision-exact: each implementation against the restatement
                           with ITS OWN mask y > 0 forced
  mask                     differs from fp64's only where |pre64| <= 1e-5 (|gamma xh| + |beta| + |r|), on <= 0.1 % of elements
Each case is evaluated once (evaluate(): one fp64 reference, every figure of the tests below) and the tests read the record."""
import copy
import functools
import random

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import encoder_glue_cases as R
from tests.glue_sweep_cases import placed

pytestmark = pytest.mark.gpu
VAR_GATE = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


def _cases():
    from mal_amd import build
    build.build(verbose=False)
    return R.cases()


CASES = _cases()
IDS = [R.case_id(c) for c in CASES]


def _module(C, gamma, beta, rm, rv, momentum, dev=None, dtype=torch.float32):
    bn = nn.BatchNorm2d(C, eps=R.EPS, momentum=momentum).to(dtype)
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    return bn.to(dev) if dev is not None else bn


def _aten(x, bn, r, relu):
    out = bn(x)
    if r is not None:
        out = out + r
    return F.relu(out) if relu else out


def _run(fn, x, bn, r, relu, g, place=(0, 0, 0)):
    """one training-mode call and its backward -> (y, dx, dr, dgamma, dbeta, what the node saved), the module's state advanced.
    ``place``: floats that x, the residual and the cotangent start into buffers of their own (tests/glue_sweep_cases.placed)"""
    lx = placed(x, place[0]).requires_grad_(True)
    lr = placed(r, place[1]).requires_grad_(True) if r is not None else None
    bn.weight.grad = bn.bias.grad = None
    y = fn(lx, bn, lr, relu)
    saved = y.grad_fn.saved_tensors if fn is not _aten else None  # before the backward frees them
    y.backward(placed(g, place[2]))
    return y, lx.grad, (lr.grad if lr is not None else None), bn.weight.grad.clone(), bn.bias.grad.clone(), saved


def _var_error(var, var64):
    """per channel: relative error where the fp64 variance is positive, error / eps where it is exactly zero"""
    var, var64 = var.double().cpu(), var64.double().cpu()
    err = (var - var64).abs()
    return float(torch.where(var64 > 0, err / var64.clamp_min(1e-300), err / R.EPS).max())


@functools.lru_cache(None)
def evaluate(case, place=(0, 0, 0), make=R.make_inputs):
    """``place`` puts the kernels' operands off the 16-byte grid (_run; ATen's run stays where it is), ``make`` builds the inputs"""
    from mal_amd.glue import bn_join, bn_join_fallback_reason
    dev = torch.device("cuda:0")
    (B, C, H, W), mode, mean = case
    relu, N = R.relu_of(mode), B * H * W
    x, r, g, gamma, beta, rm, rv = make(case)
    d = lambda t: None if t is None else t.to(dev)
    px, pr = placed(d(x), place[0]), (None if r is None else placed(d(r), place[1]))
    x64, r64, g64, gamma64, beta64 = (None if t is None else t.double() for t in (x, r, g, gamma, beta))
    m64, v64 = R.statistics(x64)
    y64, pre64, xh64 = R.forward(x64, r64, gamma64, beta64, relu, m64, v64)
    rec = {}
    # ---- forward and backward, twice (determinism), momentum 0.1
    runs = []
    for _ in range(2):
        bn = _module(C, gamma, beta, rm, rv, 0.1, dev)
        y, dx, dr, dw, db, saved = _run(bn_join, d(x), bn, d(r), relu, d(g), place)
        runs.append((y.detach(), dx, dr, dw, db, saved[3], saved[4], bn.running_mean.clone(), bn.running_var.clone(),
                     bn.num_batches_tracked.clone()))
    rec["fallback"] = bn_join_fallback_reason(px, bn, pr)
    rec["deterministic"] = all((a is None and b is None) or torch.equal(a, b) for a, b in zip(*runs))
    y, dx, dr, dw, db, save_mean, save_invstd = runs[0][:7]
    rec["save_dtype"] = (save_mean.dtype, save_invstd.dtype)
    bn_a = _module(C, gamma, beta, rm, rv, 0.1, dev)
    ya, dxa, dra, dwa, dba, _ = _run(_aten, d(x), bn_a, d(r), relu, d(g))
    rec["y"], rec["y_aten"] = R.l2rel(y, y64), R.l2rel(ya, y64)
    rec["mean"] = float((save_mean.cpu() - m64).abs().max() / max(1.0, abs(mean)))
    rec["var"] = _var_error(1.0 / save_invstd.double() ** 2 - R.EPS, v64)
    # ---- the decisions
    mask, mask_a = (y > 0).cpu(), (ya.detach() > 0).cpu()
    if relu:
        v = lambda t: t.view(1, -1, 1, 1)
        differ = mask != (y64 > 0)
        room = 1e-5 * ((v(gamma64) * xh64).abs() + v(beta64).abs() + (r64.abs() if r64 is not None else 0.0))
        rec["mask_outside"] = int((differ & (pre64.abs() > room)).sum())
        rec["mask_share"] = float(differ.double().mean())
    # ---- backward, decision-exact
    for tag, got, msk in (("", (dx, dr, dw, db), mask), ("_aten", (dxa, dra, dwa, dba), mask_a)):
        ref = R.backward(g64, x64, gamma64, relu, m64, v64, mask=msk)
        for name, a, b in zip(("dx", "dr", "dgamma", "dbeta"), got, ref):
            if a is not None:
                rec[name + tag] = R.l2rel(a, b)
    const = R.special_channels(C)[2]
    if const is not None:  # var = 0: y = relu(beta + r), no NaN anywhere
        want = beta64[const] + (r64[:, const] if r64 is not None else 0.0) + torch.zeros(B, H, W, dtype=torch.float64)
        want = torch.clamp(want, min=0) if relu else want
        rec["const_y"] = float((y[:, const].double().cpu() - want).abs().max())
    rec["finite"] = all(bool(torch.isfinite(t).all()) for t in (y, dx, dr, dw, db, save_mean, save_invstd) if t is not None)
    zero = R.special_channels(C)[0]
    rec["gamma0_dx"] = float(dx[:, zero].abs().max()) if zero is not None else 0.0
    # ---- the module's state after one and two calls, with and without a graph, both momenta
    state = []
    for momentum in R.MOMENTA:
        ref = _module(C, gamma64, beta64, rm.double(), rv.double(), momentum, dtype=torch.float64)
        fused = {"grad": _module(C, gamma, beta, rm, rv, momentum, dev), "no_grad": _module(C, gamma, beta, rm, rv, momentum, dev)}
        for call in (1, 2):
            ref(x64)
            for how, bn in fused.items():
                with torch.set_grad_enabled(how == "grad"):
                    out = bn_join(px, bn, pr, relu)
                state.append(dict(momentum=momentum, call=call, how=how, has_graph=out.grad_fn is not None,
                                  rm=R.l2rel(bn.running_mean, ref.running_mean), rv=_var_error(bn.running_var, ref.running_var),
                                  nbt=int(bn.num_batches_tracked), nbt_ref=int(ref.num_batches_tracked),
                                  nbt_dtype=bn.num_batches_tracked.dtype, same_y=torch.equal(out.detach(), y)))
    rec["state"] = state
    return rec


def hold_forward(case, rec):
    """the forward's gates on a record of evaluate() -> distance / gate of each quantity"""
    assert rec["fallback"] is None
    gate = max(1e-6, 2 * rec["y_aten"])
    print(R.case_id(case), "y %.3e ATen %.3e gate %.3e | mean %.3e var %.3e" % (rec["y"], rec["y_aten"], gate, rec["mean"], rec["var"]))
    assert rec["finite"]
    assert rec["y"] <= gate
    assert rec["mean"] <= 1e-6  # |mean - mean64| / max(1, |input mean|): half an fp32 ulp of the mean is 6e-8
    assert rec["var"] <= VAR_GATE
    assert rec["save_dtype"] == (torch.float64, torch.float64)
    if "const_y" in rec:
        assert rec["const_y"] <= 1e-6, rec["const_y"]  # one fp32 rounding of beta + r (|.| < 8)
    return {"y": rec["y"] / gate, "mean": rec["mean"] / 1e-6, "var": rec["var"] / VAR_GATE}


def hold_module_state(case, rec):
    worst = {"running_var": 0.0, "running_mean": 0.0}
    for s in rec["state"]:
        print(R.case_id(case), s)
        assert s["nbt"] == s["nbt_ref"] == s["call"] and s["nbt_dtype"] == torch.int64
        assert s["rv"] <= VAR_GATE and s["rm"] <= 1e-5
        assert s["has_graph"] == (s["how"] == "grad")
        assert s["same_y"]  # neither the momentum nor the second call of the same module changes y
        worst = {"running_var": max(worst["running_var"], s["rv"] / VAR_GATE), "running_mean": max(worst["running_mean"], s["rm"] / 1e-5)}
    return worst


def hold_backward(case, rec):
    (B, C, H, W), mode, mean = case
    names = ["dx", "dgamma", "dbeta"] + (["dr"] if mode == "residual_relu" else [])
    worst = {}
    for name in names:
        gate = max(1e-4, 1.25 * rec[name + "_aten"])
        print(R.case_id(case), "%-6s %.3e ATen %.3e gate %.3e" % (name, rec[name], rec[name + "_aten"], gate))
        assert rec[name] <= gate, name
        worst[name] = rec[name] / gate
    assert rec["gamma0_dx"] == 0.0
    if R.relu_of(mode):
        print(R.case_id(case), "mask: differs on %.3e of the elements, %d outside the room" % (rec["mask_share"], rec["mask_outside"]))
        assert rec["mask_outside"] == 0 and rec["mask_share"] <= 1e-3
        worst["mask_share"] = rec["mask_share"] / 1e-3
    return worst


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward(case):
    hold_forward(case, evaluate(case))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_module_state(case):
    hold_module_state(case, evaluate(case))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_decision_exact(case):
    hold_backward(case, evaluate(case))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_two_runs_give_the_same_bits(case):
    assert evaluate(case)["deterministic"]


# ------------------------------------------------------------------------------------------- eval mode, gradient pruning
@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ((2, 5, 3, 7), (3, 64, 6, 20))], ids=R.case_id)
def test_eval_mode(case):
    from mal_amd.glue import bn_join
    dev = torch.device("cuda:0")
    (B, C, H, W), mode, mean = case
    relu = R.relu_of(mode)
    x, r, g, gamma, beta, rm, rv = R.make_inputs(case)
    d = lambda t: None if t is None else t.to(dev)
    y64 = R.forward(x.double(), None if r is None else r.double(), gamma.double(), beta.double(), relu, rm.double(), rv.double())[0]
    bn, bn_a = _module(C, gamma, beta, rm, rv, 0.1, dev).eval(), _module(C, gamma, beta, rm, rv, 0.1, dev).eval()
    with torch.no_grad():
        y = bn_join(d(x), bn, d(r), relu)
        ya = _aten(d(x), bn_a, d(r), relu)
    own, got = R.l2rel(ya, y64), R.l2rel(y, y64)
    print(R.case_id(case), "eval y %.3e ATen %.3e" % (got, own))
    assert got <= max(1e-6, 2 * own)
    assert y.grad_fn is None
    # no side effects
    assert torch.equal(bn.running_mean.cpu(), rm) and torch.equal(bn.running_var.cpu(), rv) and int(bn.num_batches_tracked) == 0
    # with a gradient asked for, eval mode is ATen's: bit for bit, and differentiable
    lx = d(x).requires_grad_(True)
    z = bn_join(lx, bn, d(r), relu)
    la = d(x).requires_grad_(True)
    za = _aten(la, bn_a, d(r), relu)
    assert z.grad_fn is not None and torch.equal(z, za)
    z.backward(d(g)), za.backward(d(g))
    assert torch.equal(lx.grad, la.grad) and torch.equal(bn.weight.grad, bn_a.weight.grad)


def test_only_the_requested_gradients_are_computed():
    from mal_amd.glue import bn_join, bn_join_bwd
    dev = torch.device("cuda:0")
    case = ((3, 64, 6, 20), "residual_relu", 0.0)
    x, r, g, gamma, beta, rm, rv = (t.to(dev) for t in R.make_inputs(case))
    full = _run(bn_join, x, _module(64, gamma, beta, rm, rv, 0.1, dev), r, True, g)
    for need_x, need_r in ((False, True), (True, False), (False, False)):
        bn = _module(64, gamma, beta, rm, rv, 0.1, dev)
        lx, lr = x.clone().requires_grad_(need_x), r.clone().requires_grad_(need_r)
        y = bn_join(lx, bn, lr, True)
        y.backward(g)
        assert (lx.grad is None) == (not need_x) and (lr.grad is None) == (not need_r)
        if need_x:
            assert torch.equal(lx.grad, full[1])
        if need_r:
            assert torch.equal(lr.grad, full[2])
        assert torch.equal(bn.weight.grad, full[3]) and torch.equal(bn.bias.grad, full[4])
    # the operator itself: a gradient that is not asked for is None
    bn = _module(64, gamma, beta, rm, rv, 0.1, dev)
    y = bn_join(x.clone().requires_grad_(True), bn, r, True)
    sx, sy, sw, sm, si = y.grad_fn.saved_tensors
    dx, dr, dw, db = bn_join_bwd(g, sx, sy, sw, sm, si, True, need_x=False, need_r=True, need_w=False, need_b=False)
    assert dx is None and dw is None and db is None and torch.equal(dr, full[2])
    dx, dr, dw, db = bn_join_bwd(g, sx, sy, sw, sm, si, True, need_x=True, need_r=False, need_w=False, need_b=True)
    assert dr is None and dw is None and torch.equal(dx, full[1]) and torch.equal(db, full[4])
    # without the ReLU the output is not saved, and dr is the cotangent itself
    y = bn_join(x.clone().requires_grad_(True), bn, r, False)
    assert y.grad_fn.saved_tensors[1] is None
    # one value per channel in training mode: PyTorch's own error
    with pytest.raises(ValueError):
        bn_join(torch.rand(1, 4, 1, 1, device=dev), nn.BatchNorm2d(4).to(dev))
    # writing y in place afterwards is refused by autograd, not silently wrong
    lx = x.clone().requires_grad_(True)
    y = bn_join(lx, _module(64, gamma, beta, rm, rv, 0.1, dev), None, True)
    y.add_(1.0)
    with pytest.raises(RuntimeError):
        y.sum().backward()


def test_fallbacks_run_the_modules_own_composition():
    from mal_amd.glue import bn_join
    dev = torch.device("cuda:0")
    x = torch.randn(2, 6, 4, 4, generator=torch.Generator().manual_seed(1)).to(dev)
    r = torch.randn(2, 6, 4, 4, generator=torch.Generator().manual_seed(2)).to(dev)
    for make, xin in ((lambda: nn.BatchNorm2d(6, momentum=None), x), (lambda: nn.BatchNorm2d(6, track_running_stats=False), x),
                      (lambda: nn.BatchNorm2d(6, affine=False), x), (lambda: nn.BatchNorm2d(6), x.to(memory_format=torch.channels_last)),
                      (lambda: nn.BatchNorm2d(6).double(), x.double())):
        torch.manual_seed(0)
        a, b = make().to(dev), make().to(dev)
        rr = r.to(xin.dtype)
        got, ref = bn_join(xin, a, rr, True), F.relu(b(xin) + rr)
        assert torch.equal(got, ref)
        for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
            assert torch.equal(va, vb), ka


# ------------------------------------------------------------------------------------------------------------ networks
class _Deterministic:
    """MIOpen's deterministic solvers and no TF32: equal inputs give equal convolutions (tests/test_gpu_decoder_glue.py)"""

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


def _compare_models(make, call, n_out, monkeypatch=None):
    """fused and unfused fp32 copies on the device against the same model in fp64 on the CPU: outputs, parameter gradients and
    the batch-norm buffers after the forward"""
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    exact = make().double()
    for m in exact.modules():  # norms that do something: the initial gamma = 1, beta = 0 hides a swapped pair
        if isinstance(m, nn.BatchNorm2d):
            with torch.no_grad():
                m.weight.uniform_(0.5, 1.5), m.bias.uniform_(-0.3, 0.3)
    plain, fused = make().float(), make().float()
    plain.load_state_dict(exact.state_dict()), fused.load_state_dict(exact.state_dict())
    plain.to(dev), fused.to(dev)
    fused.fused_glue = True
    assert any(getattr(m, "fused_glue", False) for m in fused.modules()) and not any(getattr(m, "fused_glue", False) for m in plain.modules())
    res = {}
    with _Deterministic():
        for tag, model, dt, where in (("exact", exact, torch.float64, "cpu"), ("plain", plain, torch.float32, dev), ("fused", fused, torch.float32, dev)):
            model.train()
            outs = call(model, dt, where)
            assert len(outs) == n_out
            gen = torch.Generator().manual_seed(9)
            loss = sum((o * torch.randn(o.shape, generator=gen, dtype=torch.float64).to(o)).sum() for o in outs)
            loss.backward()
            rec = {"out_%d" % i: o.detach() for i, o in enumerate(outs)}
            rec.update({"grad:" + k: p.grad for k, p in model.named_parameters() if p.grad is not None})
            rec.update({"buf:" + k: b.clone() for k, b in model.named_buffers()})
            res[tag] = rec
    assert set(res["fused"]) == set(res["plain"]) == set(res["exact"])
    worst = 0.0
    for k in sorted(res["exact"]):
        ref = res["exact"][k]
        if k.endswith("num_batches_tracked"):
            assert torch.equal(res["fused"][k].cpu(), ref) and int(ref) >= 1, k
            continue
        if k.startswith("buf:") and k.endswith("running_var"):
            assert _var_error(res["fused"][k], ref) <= VAR_GATE, k
            continue
        own, got = R.l2rel(res["plain"][k], ref), R.l2rel(res["fused"][k], ref)
        gate = 1e-5 if k.startswith("buf:") else max(1e-4, 1.25 * own)
        worst = max(worst, got / gate)
        print("%-44s unfused %.3e fused %.3e gate %.3e" % (k, own, got, gate))
        assert got <= gate, (k, got, own)
    return worst


def _image(B, C, H, W, seed, dt, where):
    return torch.rand(B, C, H, W, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dt).to(where)


@pytest.mark.parametrize("downsample", [False, True, "kernel"], ids=["identity", "downsample", "downsample-in-the-kernel"])
def test_basic_block(downsample, monkeypatch):
    from mal_amd import networks
    if downsample == "kernel":  # the downsample norm of a map this small is ATen's by measurement: send it to the kernel too
        monkeypatch.setattr(networks, "PLAIN_JOIN_MIN_ELEMS", 0)

    def make():
        if downsample:
            return networks.BasicBlock(8, 16, 2, nn.Sequential(nn.Conv2d(8, 16, 1, 2, bias=False), nn.BatchNorm2d(16)))
        return networks.BasicBlock(8, 8)

    def call(model, dt, where):
        x = (_image(2, 8, 16, 32, 3, dt, where) - 0.5).requires_grad_(True)
        return [model(x)]

    _compare_models(make, call, 1)


def test_resnet_encoder():
    from mal_amd import networks
    _compare_models(lambda: networks.ResnetEncoder(18, False), lambda model, dt, where: model(_image(2, 3, 32, 64, 4, dt, where)), 5)


def test_resnet_encoder_matching(monkeypatch):
    from mal_amd import networks
    monkeypatch.setattr(networks.costvol, "cost_volume_outputs", _fixed_cost_volume)

    def call(model, dt, where):
        cur = _image(2, 3, 32, 64, 4, dt, where)
        look = _image(2, 3, 32, 64, 6, dt, where).view(2, 1, 3, 32, 64)
        eye = torch.eye(4, dtype=dt, device=where).expand(2, 4, 4)
        feats, low, conf = model(cur, look, eye.unsqueeze(1), eye, eye, min_depth_bin=0.1, max_depth_bin=20.0)
        return feats  # every norm of layer0 and layer1 ran twice: the current image, then the lookup frame without a graph

    _compare_models(lambda: networks.ResnetEncoderMatching(18, False, 32, 64, adaptive_bins=True, num_depth_bins=8), call, 5)


# ------------------------------------------------------------------------------------------------------------ harness
def test_harness_with_the_fused_encoder(tmp_path):
    from mal_amd import harness
    dev = torch.device("cuda:0")
    kw = dict(batch_size=2, height=96, width=160, no_matching_augmentation=True)
    random.seed(3)
    torch.manual_seed(3)
    plain = harness.TrainHarness(harness.default_options(**kw), dev)
    fused = harness.TrainHarness(harness.default_options(fused_encoder=True, **kw), dev)
    for enc in (fused.model.encoder, fused.model.mono_encoder, fused.model.pose_encoder):
        assert enc.fused_glue
    for enc in (plain.model.encoder, plain.model.mono_encoder, plain.model.pose_encoder):
        assert not enc.fused_glue
    inputs = harness.synthetic_inputs(fused.opt, dev, seed=7)
    with _Deterministic():
        for _ in range(2):
            losses = fused.train_step(copy.copy(inputs))
            assert bool(torch.isfinite(losses["loss"]).all()), losses["loss"]
    nbt = [int(b) for k, b in fused.model.named_buffers() if k.endswith("num_batches_tracked")]
    assert min(nbt) >= 2  # every norm ran in both steps, on the device
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir()
    fused.save(str(tmp_path / "a"))
    plain.model.load_state_dict(torch.load(str(tmp_path / "a" / "model.pth"), map_location="cpu"), strict=True)
    plain.load(str(tmp_path / "a"))  # a checkpoint written with the option loads without it
    for (ka, va), (kb, vb) in zip(fused.model.state_dict().items(), plain.model.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    plain.model.load_state_dict(fused.model.state_dict(), strict=True)
    with _Deterministic():
        plain.train_step(copy.copy(inputs))
    plain.save(str(tmp_path / "b"))
    fused.model.load_state_dict(torch.load(str(tmp_path / "b" / "model.pth"), map_location="cpu"), strict=True)
    fused.load(str(tmp_path / "b"))  # and the other way round
    for (ka, va), (kb, vb) in zip(plain.model.state_dict().items(), fused.model.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    fused.model.load_state_dict(plain.model.state_dict(), strict=True)
