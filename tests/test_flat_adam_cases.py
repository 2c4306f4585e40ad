"""CPU: the restatement of the flat Adam step (tests/flat_adam_restated.py) against torch.optim.Adam, both measured from the fp64
recurrence; mal_adam_plan (pure host code) replayed on the host over the case table of tests/flat_adam_cases.py; the argument
checks of mal_adam_flat / mal_adam_plan (no device is touched); and what needs no device of the Python layer
(mal_amd.optim.FlatAdam): refusals by name, the CPU step's error, the checkpoint interchange with torch.optim.Adam and the
harness switch."""
import ctypes
import os
import re

import pytest
import torch

from tests import flat_adam_cases as T
from tests import flat_adam_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from mal_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


# ---------------------------------------------------------------------------------------------- restatement against torch
def _distances(n, steps, scale):
    """per quantity (restatement's, torch.optim.Adam's) L2-relative distance from the fp64 recurrence"""
    p0, grads = T.gate_case(n, steps, scale)
    p64, m64, v64 = R.run64(p0, grads)
    p32, m32, v32 = R.run32(p0, grads)
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([pt], lr=1e-3)
    for g in grads:
        pt.grad = g.clone()
        opt.step()
    st = opt.state[pt]
    p0d = p0.double()
    return {"update": (R.rel_l2(p32.double() - p0d, p64 - p0d), R.rel_l2(pt.detach().double() - p0d, p64 - p0d)),
            "m": (R.rel_l2(m32, m64), R.rel_l2(st["exp_avg"], m64)),
            "v": (R.rel_l2(v32, v64), R.rel_l2(st["exp_avg_sq"], v64))}


def test_restatement_is_as_close_to_fp64_as_torch_adam():
    """NOT a bitwise gate (torch's CPU kernels fuse multiply-adds in their vectorised bodies only): per tensor, the
    restatement's distance from the fp64 recurrence over torch.optim.Adam's own, for the accumulated update, m and v.
    Measured here over GATE_CASES: at most 1.0027 (update), 1.2016 (m), 1.0583 (v); gated at 1.25 x that."""
    worst = {k: 0.0 for k in T.GATE_RATIO}
    for n, steps, scale in T.GATE_CASES:
        d = _distances(n, steps, scale)
        for k, (mine, theirs) in d.items():
            assert theirs > 0 and mine > 0
            worst[k] = max(worst[k], mine / theirs)
            print("n=%d steps=%d scale=%g %s: restated %.4g torch %.4g ratio %.4f" % (n, steps, scale, k, mine, theirs, mine / theirs))
            assert mine / theirs <= T.GATE_RATIO[k], (n, steps, scale, k, mine, theirs)
            # and both are rounding-level: fp32 state against fp64 (the update carries the rounding of p itself, ~1e-3 of it)
            assert mine < (1e-4 if k == "update" else 1e-6)
    print("largest ratios:", worst)


def test_restatement_is_one_rounding_per_operator():
    """the same chain in numpy float32 scalars-and-arrays arithmetic (IEEE operations, correctly rounded square root) gives
    the same bits at a size where torch's own fp32 CPU sqrt does not (it is why the restatement takes its root in fp64)"""
    import numpy as np
    rng = np.random.default_rng(0)
    n, f = 50000, np.float32
    for scale, t in ((1e-6, 1), (1.0, 3), (30.0, 1000)):
        p, g = rng.standard_normal(n).astype(f), (rng.standard_normal(n) * scale).astype(f)
        m, v = (rng.standard_normal(n) * scale * 0.1).astype(f), (rng.random(n) * scale * scale * 0.01).astype(f)
        c1, b2, c2, bs, e, a = (f(x) for x in R.scalars(1e-3, (0.9, 0.999), 1e-8, t))
        m1 = m + (g - m) * c1
        v1 = v * b2 + (c2 * g) * g
        p1 = p + a * (m1 / (np.sqrt(v1) / bs + e))
        tp, tm, tv = R.step32(*(torch.from_numpy(x) for x in (p, g, m, v)), t)
        for mine, want in ((tp, p1), (tm, m1), (tv, v1)):
            assert mine.dtype == torch.float32 and np.array_equal(mine.numpy().view(np.int32), want.view(np.int32))


def test_restatement_handles_the_special_values():
    """zeros stay put, |g| = 1e-23 underflows in v exactly as fp32 does, inf and NaN gradients poison their own element only"""
    p0 = torch.linspace(-1, 1, 8)
    g = torch.tensor([0.0, -0.0, 1e-23, -1e-23, float("inf"), float("nan"), 1.0, -30.0])
    p, m, v = R.run32(p0, [g])
    assert torch.equal(p[:2], p0[:2]) and float(m[:2].abs().sum()) == 0 and float(v[:2].abs().sum()) == 0
    assert float(v[2]) == 0.0 and float(m[2]) != 0.0  # (c2 * g) * g underflows to zero; m does not
    assert torch.isnan(p[4]) and torch.isnan(p[5]) and torch.isfinite(p[[0, 1, 2, 3, 6, 7]]).all()
    assert float(m[4]) == float("inf") and torch.isnan(m[5])


# ------------------------------------------------------------------------------------------------------------- symbols
def test_symbols_header_and_sources(lib):
    from mal_amd import build, _lib
    header = open(os.path.join(ROOT, "include", "mal_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for sym in ("mal_adam_flat", "mal_adam_plan"):
        assert re.search(r"\bint %s\(" % sym, header) and sym in _lib.SIGNATURES and hasattr(raw, sym), sym
    assert "} mal_adam_chunk;" in header and "mal_adam.hip" in build.SOURCES
    from mal_amd.optim import adam_plan
    assert adam_plan(1, 1)["chunk_bytes"] == ctypes.sizeof(_lib.AdamChunk) == 16


# ---------------------------------------------------------------------------------------------------------------- plan
def _tables():
    from mal_amd import harness, networks
    tabs = {name: list(sizes) for name, sizes in T.ORDERINGS.items()}
    tabs["repdepth_like_120"] = T.repdepth_like_120()
    tabs["repdepth"] = [p.numel() for p in networks.RepDepth(harness.default_options()).parameters() if p.requires_grad]
    tabs["past_one_window"] = [1 + (i * 7) % 13 for i in range(T.WINDOW + 44)]
    return tabs


def test_case_table_hits_every_residue():
    assert all(sorted(o) == sorted(T.SIZES) for o in T.ORDERINGS.values()) and len(T.ORDERINGS) >= 2
    assert {off % 4 for off in T.offsets(T.ORDERINGS["mixed"])} == {0, 1, 2, 3}
    long_at = {T.offsets(o)[o.index(4099)] % 4 for o in T.ORDERINGS.values()}
    assert long_at == {0, 1, 2, 3}
    assert len(T.repdepth_like_120()) == 120 and 1 in T.repdepth_like_120()


def test_plan_covers_every_element_exactly_once(lib):
    from mal_amd.optim import adam_plan
    for name, sizes in _tables().items():
        offs = T.offsets(sizes)
        ranges = [(0, len(sizes))]
        if len(sizes) <= 16:
            ranges += [(0, 3), (3, 4), (7, len(sizes) - 7), (2, 1), (4, 0)]
        for first, count in ranges:
            total = sum(sizes[first:first + count])
            pl = adam_plan(max(count, 1), total)
            assert (pl["threads"], pl["tile_elements"], pl["table_window"]) == (T.THREADS, T.TILE, T.WINDOW)
            assert pl["blocks"] == min(T.MAX_BLOCKS, -(-total // T.TILE) + max(count, 1)) and pl["blocks"] >= 1
            if name == "repdepth" and total > 2 ** 22:
                # the whole model: 41.2 M elements; replaying 2048 workgroups over them is done once, with the capped grid
                assert pl["blocks"] == T.MAX_BLOCKS
            for residue in ((0, 1) if len(sizes) <= 16 else (0,)):
                touched, tiles, owners = T.cover(sizes, offs, first, count, pl["blocks"], residue)
                for e, c in enumerate(touched):
                    want = 1 if first <= e < first + count else 0
                    assert bool((c == want).all()), (name, first, count, e, residue)
                # every tile has exactly one owner, and the bound the grid is sized by holds
                assert sum(len(o) for o in owners) == tiles <= -(-total // T.TILE) + count
                assert len(set().union(*owners)) == tiles
                if tiles >= pl["blocks"]:  # enough tiles: no workgroup is idle and the load is even to within one tile
                    assert max(len(o) for o in owners) - min(len(o) for o in owners) <= 1


def test_invalid_arguments_are_refused_without_a_device(lib):
    p, n, E = 4096, None, -1  # a non-null "pointer" that is never dereferenced: every call below returns before any HIP call
    ok = dict(table=p, n_chunks=10, first=0, count=10, range_elements=5584, grad=p, exp_avg=p, exp_avg_sq=p, flat_elements=5584,
              t=1, c1=0.1, beta2=0.999, c2=0.001, bs=0.0316, eps=1e-8, a=-1e-2, zero_grad=0)

    def f(**kw):
        a = dict(ok, **kw)
        return lib.mal_adam_flat(a["table"], a["n_chunks"], a["first"], a["count"], a["range_elements"], a["grad"], a["exp_avg"],
                                 a["exp_avg_sq"], a["flat_elements"], a["t"], a["c1"], a["beta2"], a["c2"], a["bs"], a["eps"],
                                 a["a"], a["zero_grad"], n)

    for name in ("table", "grad", "exp_avg", "exp_avg_sq"):
        assert f(**{name: n}) == E, name
    for bad in (dict(first=-1), dict(count=-1), dict(first=11), dict(first=10, count=1), dict(first=3, count=8), dict(n_chunks=0),
                dict(first=2 ** 31 - 1, count=2 ** 31 - 1),
                dict(t=0), dict(t=-5), dict(bs=0.0), dict(bs=-0.5), dict(bs=float("inf")), dict(bs=float("nan")),
                dict(flat_elements=0), dict(flat_elements=2 ** 31), dict(range_elements=2 ** 31, flat_elements=2 ** 33),
                dict(range_elements=-1), dict(range_elements=5585), dict(grad=4098), dict(exp_avg=4097), dict(table=4100)):
        assert f(**bad) == E, bad
    assert f(first=10, count=0) == 0 and f(first=4, count=0) == 0  # an empty range inside the table: nothing to do, no launch
    outs = [ctypes.c_int(0) for _ in range(5)]
    refs = [ctypes.byref(o) for o in outs]
    assert lib.mal_adam_plan(0, 10, *refs) == E and lib.mal_adam_plan(-1, 10, *refs) == E
    assert lib.mal_adam_plan(3, -1, *refs) == E and lib.mal_adam_plan(3, 2 ** 31, *refs) == E
    assert lib.mal_adam_plan(3, 2 ** 31 - 1, *refs) == 0 and outs[0].value == T.MAX_BLOCKS  # just below 2^31
    assert lib.mal_adam_plan(3, 0, *refs) == 0 and outs[0].value == 3
    assert lib.mal_adam_plan(3, 10, None, None, None, None, None) == 0


# -------------------------------------------------------------------------------------------------------- Python layer
def _cpu_setup(sizes=(5, 12, 1, 64), seed=0):
    from mal_amd import dp
    gen = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(n, generator=gen).reshape(-1, 1) if n % 2 else torch.randn(n, generator=gen))
              for n in sizes]
    return params, dp.FlatGradBucket(params)


def test_unsupported_flavours_are_refused_by_name():
    from mal_amd.optim import FlatAdam
    params, bucket = _cpu_setup()
    for kw, name in ((dict(weight_decay=1e-4), "weight_decay"), (dict(amsgrad=True), "amsgrad"), (dict(maximize=True), "maximize"),
                     (dict(capturable=True), "capturable"), (dict(differentiable=True), "differentiable")):
        with pytest.raises(NotImplementedError, match=name):
            FlatAdam(params, bucket, 1e-3, **kw)
    opt = FlatAdam(params, bucket, 1e-3)
    sd = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in params], amsgrad=True).state_dict()
    with pytest.raises(NotImplementedError, match="amsgrad"):
        opt.load_state_dict(sd)
    with pytest.raises(ValueError):
        FlatAdam(params[:2], bucket)          # not the bucket's list
    with pytest.raises(ValueError):
        FlatAdam(params[::-1], bucket)        # not its order
    with pytest.raises(ValueError):
        opt.zero_grad(set_to_none=True)       # would drop the views
    opt.zero_grad()
    assert bucket.check_views()


def test_cpu_step_raises_naming_the_device():
    from mal_amd import _lib
    from mal_amd.optim import FlatAdam
    params, bucket = _cpu_setup()
    opt = FlatAdam(params, bucket, 1e-3)
    before = [p.detach().clone() for p in params]
    bucket.flat.fill_(1.0)
    with pytest.raises(_lib.MalError, match="CUDA/HIP"):
        opt.step()
    with pytest.raises(_lib.MalError, match="CUDA/HIP"):
        opt.step(zero_grad=True)
    assert opt.t == 0 and all(torch.equal(a, p.detach()) for a, p in zip(before, params))  # no CPU fallback, nothing moved
    assert float(bucket.flat.sum()) == bucket.flat.numel()


def test_param_group_has_torchs_keys_and_schedulers_drive_lr():
    from mal_amd import harness
    from mal_amd.optim import FlatAdam
    params, bucket = _cpu_setup()
    opt = FlatAdam(params, bucket, 2e-4, betas=(0.8, 0.99), eps=1e-7)
    ref = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in params], 2e-4, betas=(0.8, 0.99), eps=1e-7)
    assert len(opt.param_groups) == 1 and set(opt.param_groups[0]) == set(ref.param_groups[0])
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["amsgrad"]) == (2e-4, (0.8, 0.99), 1e-7, 0, False)
    assert all(a is b for a, b in zip(g["params"], params))
    sched = torch.optim.lr_scheduler.StepLR(opt, 1, 0.1)
    opt._opt_called = True  # what a step would set: keeps the scheduler's order warning quiet on the CPU, where step() raises
    sched.step()
    assert abs(opt.param_groups[0]["lr"] - 2e-5) < 1e-12
    warm = harness.WarmupStepLRScheduler(opt, 1e-7, 2e-4, 10, 1000)
    warm.step()
    assert opt.param_groups[0]["lr"] == warm.get_last_lr()[0] != 2e-5
    g["weight_decay"] = 0.1  # a flavour switched on behind the constructor's back is refused at the step, before the device check
    with pytest.raises(NotImplementedError, match="weight_decay"):
        opt.step()


def test_state_dict_interchange_with_torch_adam(tmp_path):
    from mal_amd.optim import FlatAdam
    sizes = (5, 12, 1, 64, 4099)
    params, bucket = _cpu_setup(sizes)
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in params]
    ref = torch.optim.Adam(theirs, 3e-4, betas=(0.85, 0.98), eps=1e-6)
    gen = torch.Generator().manual_seed(5)
    for _ in range(3):
        for p in theirs:
            p.grad = torch.randn(p.shape, generator=gen)
        ref.step()
    sd = ref.state_dict()
    opt = FlatAdam(params, bucket, 1e-3)
    assert opt.state_dict()["state"] == {} and opt.t == 0  # before the first step: empty, as torch's
    torch.save(sd, tmp_path / "adam.pth")
    opt.load_state_dict(torch.load(tmp_path / "adam.pth", map_location="cpu"))
    assert opt.t == 3
    back = opt.state_dict()
    assert set(back) == set(sd) and sorted(back["state"]) == sorted(sd["state"]) == list(range(len(sizes)))
    for i, p in enumerate(params):
        a, b = back["state"][i], sd["state"][i]
        assert set(a) == set(b) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(a["step"]) == float(b["step"]) == 3.0 and a["step"].dtype == b["step"].dtype and a["step"].shape == b["step"].shape
        for k in ("exp_avg", "exp_avg_sq"):
            assert a[k].shape == p.shape and torch.equal(a[k], b[k])
            assert a[k].data_ptr() != opt.exp_avg.data_ptr() and a[k]._base is None  # copies, not views of the flat buffers
    assert len(back["param_groups"]) == 1 and set(back["param_groups"][0]) == set(sd["param_groups"][0])
    for k, v in sd["param_groups"][0].items():
        assert back["param_groups"][0][k] == v, k       # lr, betas, eps travelled; params are the indices 0..n-1
    assert opt.param_groups[0]["lr"] == 3e-4 and tuple(opt.param_groups[0]["betas"]) == (0.85, 0.98)
    assert bucket.check_views()                          # loading replaced no gradient view
    # the moments sit at the bucket's offsets in the flat buffers
    off = 0
    for i, p in enumerate(params):
        assert torch.equal(opt.exp_avg[off:off + p.numel()].view_as(p), sd["state"][i]["exp_avg"])
        off += p.numel()
    # the reverse direction: torch.optim.Adam takes FlatAdam's dictionary and steps on from it exactly as from its own
    torch.save(back, tmp_path / "flat.pth")
    again = [torch.nn.Parameter(p.detach().clone()) for p in theirs]
    ref2 = torch.optim.Adam(again, 1e-3)
    ref2.load_state_dict(torch.load(tmp_path / "flat.pth", map_location="cpu"))
    for a, b in zip(theirs, again):
        a.grad = torch.randn(a.shape, generator=gen)
        b.grad = a.grad.clone()
    ref.step()
    ref2.step()
    assert all(torch.equal(a, b) for a, b in zip(theirs, again))
    assert float(ref2.state[again[0]]["step"]) == 4.0
    # an empty dictionary (a fresh torch.optim.Adam's) resets
    opt.load_state_dict(torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in params]).state_dict())
    assert opt.t == 0 and float(opt.exp_avg.abs().sum()) == 0 and float(opt.exp_avg_sq.abs().sum()) == 0
    # what cannot be represented is refused: differing step numbers, wrong shapes
    bad = ref.state_dict()
    bad["state"][1]["step"] = torch.tensor(9.0)
    with pytest.raises(ValueError, match="step"):
        opt.load_state_dict(bad)
    other = FlatAdam(*_cpu_setup((5, 12, 1, 64, 4098)))
    with pytest.raises(ValueError, match="shape"):
        other.load_state_dict(sd)


def test_harness_switch_is_off_by_default_and_independent():
    from mal_amd import dp, harness
    assert harness.default_options().fused_adam is False
    on = harness.default_options(fused_adam=True)
    assert on.fused_adam is True and (on.fused_decoder, on.fused_encoder, on.fused_pool) == (False, False, False)
    for other in ("fused_decoder", "fused_encoder", "fused_pool"):
        assert harness.default_options(**{other: True}).fused_adam is False
    # begin_step's keyword: the default zeroes as it always did, zero=False leaves the buffer to the caller
    params, bucket = _cpu_setup()
    bucket.flat.fill_(2.0)
    bucket.begin_step(zero=False)
    assert float(bucket.flat.sum()) == 2.0 * bucket.flat.numel()
    bucket.begin_step()
    assert float(bucket.flat.abs().sum()) == 0
    # the harness builds FlatAdam only when asked (CPU construction works; the update itself needs the device)
    kw = dict(batch_size=1, height=64, width=64)
    plain = harness.TrainHarness(harness.default_options(**kw), "cpu")
    fused = harness.TrainHarness(harness.default_options(fused_adam=True, **kw), "cpu")
    from mal_amd.optim import FlatAdam
    assert type(plain.optimizer) is torch.optim.Adam and type(fused.optimizer) is FlatAdam
    assert fused.optimizer.bucket is fused.bucket and fused.bucket.check_views() and plain.bucket.check_views()
    assert fused.optimizer.param_groups[0]["lr"] == plain.optimizer.param_groups[0]["lr"] == 1e-4
    assert isinstance(fused.scheduler, torch.optim.lr_scheduler.StepLR)
