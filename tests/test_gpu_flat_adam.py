"""GPU: mal_amd.optim.FlatAdam (mal_amd/csrc/mal_adam.hip) over the case table of tests/flat_adam_cases.py.

Truth is the fp32 restatement (tests/flat_adam_restated.py; tests/test_flat_adam_cases.py holds it to torch.optim.Adam and the
fp64 recurrence on the CPU): the kernel agrees with it BIT FOR BIT in p, m and v -- NaNs by position -- at every chunk size,
offset residue and gradient content of the table, with and without zero_grad, whole and in sub-ranges, run after run.  Then
the harness with fused_adam=True: one real step by hand against the restatement, and checkpoints both ways."""
import random

import pytest
import torch

from tests import flat_adam_cases as T
from tests import flat_adam_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILLINGS = ("scale_1e-6", "scale_1", "scale_30", "zeros", "tiny", "inf_nan")
LRS = (1e-3, 1e-3, 2.5e-4)  # the learning rate changes between the second and the third step


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


def gradients(filling, n, gen):
    if filling.startswith("scale_"):
        return torch.randn(n, generator=gen) * float(filling[6:])
    if filling == "zeros":
        z = torch.zeros(n)
        z[1::2] = -0.0
        return z
    if filling == "tiny":  # (c2 * g) * g: 1e-23 -> 0, 3e-21 and 1e-20 -> denormals; m stays normal or denormal
        mag = torch.tensor([1e-23, 3e-21, 1e-20, 1e-23])[torch.randint(0, 4, (n,), generator=gen)]
        return mag * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)
    g = torch.randn(n, generator=gen)
    g[int(torch.randint(0, n, (1,), generator=gen))] = float("inf")
    g[n // 2] = float("nan")
    g[n - 1] = float("-inf")
    return g


def setup(sizes, seed, dev=DEV):
    """parameters as separate allocations (odd sizes as (n, 1) tensors), their bucket and optimizer; the CPU copy of p0"""
    from mal_amd import dp
    from mal_amd.optim import FlatAdam
    gen = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(n, generator=gen) for n in sizes]
    params = [torch.nn.Parameter((p.reshape(-1, 1) if n % 2 else p).clone().to(dev)) for p, n in zip(p0, sizes)]
    bucket = dp.FlatGradBucket(params)
    return params, bucket, FlatAdam(params, bucket, LRS[0]), torch.cat(p0), gen


def same_bits(x, y, what=""):
    """x (GPU or CPU) and y (CPU) fp32: NaNs at the same positions, every other element the same 32 bits"""
    x, y = x.detach().reshape(-1).cpu(), y.detach().reshape(-1)
    assert x.shape == y.shape, what
    nx, ny = torch.isnan(x), torch.isnan(y)
    assert torch.equal(nx, ny), "%s: NaNs at different positions" % what
    a, b = x[~nx].view(torch.int32), y[~ny].view(torch.int32)
    bad = (a != b).nonzero().reshape(-1)
    assert bad.numel() == 0, "%s: %d of %d elements differ, first at %d: %r vs %r" % (
        what, bad.numel(), a.numel(), int(bad[0]), float(x[~nx][bad[0]]), float(y[~ny][bad[0]]))


def flat_params(params):
    return torch.cat([p.detach().reshape(-1) for p in params])


def run_case(order, filling, seed=0, zero_grad=False):
    """three steps (lr changes before the third) and one at t = 1000 from a loaded state, each checked against the restatement
    -> the device tensors after the last step"""
    sizes = T.ORDERINGS[order]
    n = sum(sizes)
    params, bucket, opt, p, gen = setup(sizes, seed)
    m, v = torch.zeros(n), torch.zeros(n)
    for k, lr in enumerate(LRS):
        g = gradients(filling, n, gen)
        bucket.flat.copy_(g)
        opt.param_groups[0]["lr"] = lr
        opt.step(zero_grad=zero_grad)
        p, m, v = R.step32(p, g, m, v, k + 1, lr)
        what = "%s/%s step %d" % (order, filling, k + 1)
        same_bits(flat_params(params), p, what + " p")
        same_bits(opt.exp_avg, m, what + " m")
        same_bits(opt.exp_avg_sq, v, what + " v")
        same_bits(bucket.flat, torch.zeros(n) if zero_grad else g, what + " g")
        assert opt.t == k + 1
    # t = 1000 from a loaded state: bias corrections near 1, moments that have seen history
    sd = opt.state_dict()
    m = torch.randn(n, generator=gen) * 0.1
    v = torch.rand(n, generator=gen) * 0.01
    off = 0
    for i, s in enumerate(sizes):
        sd["state"][i] = {"step": torch.tensor(999.0), "exp_avg": m[off:off + s].view_as(params[i]).clone(),
                          "exp_avg_sq": v[off:off + s].view_as(params[i]).clone()}
        off += s
    opt.load_state_dict(sd)
    p = torch.nan_to_num(p, nan=0.5, posinf=1.0, neginf=-1.0)  # restart the poisoned elements
    with torch.no_grad():
        off = 0
        for q, s in zip(params, sizes):
            q.copy_(p[off:off + s].view_as(q))
            off += s
    g = gradients(filling, n, gen)
    bucket.flat.copy_(g)
    opt.step(zero_grad=zero_grad)
    assert opt.t == 1000
    p, m, v = R.step32(p, g, m, v, 1000, LRS[-1])
    same_bits(flat_params(params), p, "%s/%s t=1000 p" % (order, filling))
    same_bits(opt.exp_avg, m, "%s/%s t=1000 m" % (order, filling))
    same_bits(opt.exp_avg_sq, v, "%s/%s t=1000 v" % (order, filling))
    assert bucket.check_views()
    return flat_params(params).clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()


@pytest.mark.parametrize("order", sorted(T.ORDERINGS))
def test_kernel_equals_restatement_bit_for_bit(order):
    for filling in FILLINGS:
        run_case(order, filling, seed=len(filling))


def test_zero_grad_zeroes_only_what_it_read_and_changes_nothing_else():
    for order in ("mixed", "long_at_3"):
        for filling in ("scale_1", "inf_nan"):
            plain = run_case(order, filling, seed=3)
            zeroing = run_case(order, filling, seed=3, zero_grad=True)  # checks the gradient buffer is all zero after every step
            for a, b, name in zip(plain, zeroing, "pmv"):
                same_bits(a, b.cpu(), "%s/%s %s with and without zero_grad" % (order, filling, name))
    # a launched sub-range: everything of the flat buffers and of the parameters outside it keeps a sentinel pattern
    sizes = T.ORDERINGS["mixed"]
    offs, n = T.offsets(sizes), sum(sizes)
    for first, count in ((2, 5), (0, 1), (9, 1), (1, 8)):
        params, bucket, opt, p0, gen = setup(sizes, 11)
        sentinel = (torch.arange(n, dtype=torch.float32) % 251) + 1000.0
        g = gradients("scale_1", n, gen)
        lo, hi = offs[first], offs[first + count - 1] + sizes[first + count - 1]
        inside = torch.zeros(n, dtype=torch.bool)
        inside[lo:hi] = True
        g = torch.where(inside, g, sentinel)
        bucket.flat.copy_(g)
        opt.exp_avg.copy_(sentinel)
        opt.exp_avg_sq.copy_(sentinel)
        opt.t = 1
        opt.update_range(first, count, zero_grad=True)
        p, m, v = R.step32(p0, g, sentinel, sentinel, 1, LRS[0])
        same_bits(bucket.flat, torch.where(inside, torch.zeros(n), sentinel), "sentinel g [%d,%d)" % (first, first + count))
        same_bits(opt.exp_avg, torch.where(inside, m, sentinel), "sentinel m")
        same_bits(opt.exp_avg_sq, torch.where(inside, v, sentinel), "sentinel v")
        same_bits(flat_params(params), torch.where(inside, p, p0), "sentinel p")


def test_sub_ranges_equal_one_whole_launch():
    sizes = T.ORDERINGS["long_at_2"]
    n = sum(sizes)
    for cuts in ((0, 4, 10), (0, 3, 7, 10), (0, 1, 9, 10)):
        results = []
        for split in (False, True):
            params, bucket, opt, _, gen = setup(sizes, 21)
            for k in range(2):
                bucket.flat.copy_(gradients("scale_30", n, gen))
                if not split:
                    opt.step(zero_grad=True)
                else:
                    opt.t += 1
                    for a, b in zip(cuts[:-1], cuts[1:]):
                        opt.update_range(a, b - a, zero_grad=True)
                assert float(bucket.flat.abs().sum()) == 0
            results.append((flat_params(params).cpu(), opt.exp_avg.cpu(), opt.exp_avg_sq.cpu()))
        for a, b, name in zip(results[0], results[1], "pmv"):
            same_bits(a, b, "ranges %s %s" % (cuts, name))


def test_table_longer_than_one_window_and_a_replaced_parameter():
    from mal_amd import _lib
    sizes = [1 + (i * 7) % 13 for i in range(T.WINDOW + 44)]  # 300 tiny chunks: the table passes through LDS in two windows
    n = sum(sizes)
    params, bucket, opt, p, gen = setup(sizes, 31)
    g = gradients("scale_1", n, gen)
    bucket.flat.copy_(g)
    opt.step()
    p, m, v = R.step32(p, g, torch.zeros(n), torch.zeros(n), 1, LRS[0])
    same_bits(flat_params(params), p, "two windows p")
    same_bits(opt.exp_avg, m, "two windows m")
    # a parameter's storage is replaced: the table is rebuilt, the NEW storage is updated and the old one is left alone
    old = params[5].data
    kept = old.clone()
    params[5].data = old.clone()
    opt.step()
    p, m, v = R.step32(p, g, m, v, 2, LRS[0])
    same_bits(flat_params(params), p, "replaced parameter p")
    assert torch.equal(old, kept)
    # a gradient that left the bucket cannot be mended: refused before anything is launched
    params[7].grad = None
    with pytest.raises(_lib.MalError, match="gradient of parameter 7"):
        opt.step()
    assert opt.t == 2
    same_bits(flat_params(params), p, "refused step moved nothing")


def test_both_optimizers_are_within_the_cpu_gate_of_fp64_on_the_gpu():
    """after 3 steps from the same gradients, the accumulated update of FlatAdam and of torch.optim.Adam ON THE GPU is, per
    tensor, within GATE_RATIO["update"] (the margin measured on the CPU, x 1.25) of torch.optim.Adam's CPU distance from fp64"""
    from mal_amd import dp
    from mal_amd.optim import FlatAdam
    sizes = (4096, 4099, 10000)
    gen = torch.Generator().manual_seed(77)
    p0 = [torch.randn(s, generator=gen) for s in sizes]
    grads = [[torch.randn(s, generator=gen) for s in sizes] for _ in range(3)]
    mine = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
    bucket = dp.FlatGradBucket(mine)
    opt = FlatAdam(mine, bucket, 1e-3)
    theirs = [torch.nn.Parameter(p.clone().to(DEV)) for p in p0]
    ref_gpu = torch.optim.Adam(theirs, 1e-3)
    cpu = [torch.nn.Parameter(p.clone()) for p in p0]
    ref_cpu = torch.optim.Adam(cpu, 1e-3)
    for gs in grads:
        bucket.flat.copy_(torch.cat(gs))
        opt.step(zero_grad=True)
        for q, c, g in zip(theirs, cpu, gs):
            q.grad, c.grad = g.to(DEV), g.clone()
        ref_gpu.step()
        ref_cpu.step()
    for i, p in enumerate(p0):
        p64 = R.run64(p, [gs[i] for gs in grads])[0]
        want = p64 - p.double()
        d_cpu = R.rel_l2(cpu[i].detach().double() - p.double(), want)
        d_flat = R.rel_l2(mine[i].detach().cpu().double() - p.double(), want)
        d_gpu = R.rel_l2(theirs[i].detach().cpu().double() - p.double(), want)
        print("n=%d: torch cpu %.4g, FlatAdam %.4g (x%.4f), torch gpu %.4g (x%.4f)" % (sizes[i], d_cpu, d_flat, d_flat / d_cpu, d_gpu, d_gpu / d_cpu))
        assert 0 < d_flat <= T.GATE_RATIO["update"] * d_cpu
        assert 0 < d_gpu <= T.GATE_RATIO["update"] * d_cpu


def _harness(**kw):
    from mal_amd import harness
    opt = harness.default_options(batch_size=2, height=96, width=160, **kw)
    return opt, harness.TrainHarness(opt, DEV)


def test_harness_step_by_hand_equals_the_restatement():
    from mal_amd import harness
    from mal_amd.optim import FlatAdam
    torch.manual_seed(0)
    random.seed(0)
    opt, h = _harness(fused_adam=True)
    assert type(h.optimizer) is FlatAdam
    inputs = harness.synthetic_inputs(opt, DEV, seed=3)
    h.model.train()
    h.bucket.begin_step()
    outputs, losses = h.process_batch(inputs, 0)
    losses["loss"].backward()
    h.bucket.finish()
    p0, g = flat_params(h.params).cpu(), h.bucket.flat.detach().cpu().clone()
    assert float(g.abs().sum()) > 0
    h.optimizer.step(zero_grad=True)
    n = g.numel()
    p, m, v = R.step32(p0, g, torch.zeros(n), torch.zeros(n), 1, opt.learning_rate)
    same_bits(flat_params(h.params), p, "harness p")
    same_bits(h.optimizer.exp_avg, m, "harness m")
    same_bits(h.optimizer.exp_avg_sq, v, "harness v")
    assert not torch.equal(p, p0)
    assert float(h.bucket.flat.abs().sum()) == 0 and h.bucket.check_views()
    # full steps: the first zeroes the buffer itself, the second relies on the optimizer having done it
    for _ in range(2):
        loss = h.train_step(inputs)["loss"]
        assert torch.isfinite(loss.detach()).all()
        assert float(h.bucket.flat.abs().sum()) == 0 and h.bucket.check_views()
    assert h.optimizer.t == 3 and h.step_count == 2
    h.end_epoch()  # StepLR drives the one group


def test_checkpoints_interchange_between_the_two_optimizers(tmp_path):
    from mal_amd import harness
    torch.manual_seed(1)
    random.seed(1)
    opt_f, fused = _harness(fused_adam=True)
    inputs = harness.synthetic_inputs(opt_f, DEV, seed=4)
    fused.train_step(inputs)
    fused.save(str(tmp_path / "a"))
    opt_p, plain = _harness()
    plain.load(str(tmp_path / "a"))

    def same_state(a, b, step):
        sa, sb = a.optimizer.state_dict(), b.optimizer.state_dict()
        assert sorted(sa["state"]) == sorted(sb["state"]) == list(range(len(a.params)))
        for i in sa["state"]:
            assert float(sa["state"][i]["step"]) == float(sb["state"][i]["step"]) == step
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(sa["state"][i][k].cpu(), sb["state"][i][k].cpu()), (i, k)
        assert set(sa["param_groups"][0]) == set(sb["param_groups"][0])

    same_state(fused, plain, 1.0)
    assert type(plain.optimizer) is torch.optim.Adam
    assert torch.isfinite(plain.train_step(inputs)["loss"].detach()).all()
    # and back: torch.optim.Adam's file into a fused_adam harness
    plain.save(str(tmp_path / "b"))
    _, again = _harness(fused_adam=True)
    again.load(str(tmp_path / "b"))
    same_state(plain, again, 2.0)
    assert again.optimizer.t == 2 and again.bucket.check_views()
    assert torch.isfinite(again.train_step(inputs)["loss"].detach()).all()
    assert again.optimizer.t == 3


def test_two_runs_give_the_same_bits():
    for order, filling in (("mixed", "scale_1"), ("long_at_1", "inf_nan")):
        a = run_case(order, filling, seed=9, zero_grad=True)
        b = run_case(order, filling, seed=9, zero_grad=True)
        for x, y, name in zip(a, b, "pmv"):
            same_bits(x, y.cpu(), "repeat %s/%s %s" % (order, filling, name))
