"""Which tie-break noise map reaches which pass, and the rule at exact ties -- two things the free-running and the
decision-exact parity tests cannot see.

The automask compares ``min_c r_c <= identity + 1e-5 * noise``: at that scale the noise only decides near-tie pixels, which the
free-running gates excuse and the decision-exact gates force onto the oracle.  Here the maps are LOUD (N(0,1) x F_LOUD): the
noise then decides a large share of the automask bits (each test first shows, on the oracle, that at least 20 % of the
pixels differ from the plain map's), so a pass that reads another unit's map, or none, fails the ordinary gates.

At an exact tie ``torch.min`` / ``argmin`` take the first index: frame -1.  Symmetric batches (the same image and the same
pose for frame -1 and frame +1) make the two candidates equal; frame +1 must then never win, and its pose leaves receive no
photometric gradient at all.  Disparity plateaus (blocks of exactly equal values) hold the smoothness term's sign(0) = 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from mal_amd.synthetic import make_batch
from oracle import mal_oracle as O
from tests import hip_harness as HH
from tests.test_gpu_decisions import (_dr_build, _dr_build_pu, _dr_decode, _dr_hold_against_forced_oracle, _dr_oracle_pu,
                                      _to64, check_step_decision_exact, run_step_with_decisions)
from tests.test_gpu_multiscale import check_multiscale_decision_exact

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F_LOUD = 2e4    # 1e-5 * F_LOUD * N(0,1): comparable with the reprojection error (~0.05 between r and the identity term)
POWER = 0.2     # the share of automask bits the loud map must decide on the oracle


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


def _mask(rp, ident, noise):
    """the oracle's automask (compute_loss_masks: argmin([rp, identity + 1e-5 noise]) == 0) as a bool array"""
    rp, ident, noise = (torch.as_tensor(t) for t in (rp, ident, noise))
    return (O.compute_loss_masks(rp, ident + noise * 0.00001) > 0).numpy()


def _power(rp, ident, plain):
    """share of the pixels whose automask bit the loud map decides differently from the plain one"""
    return float((_mask(rp, ident, plain) != _mask(rp, ident, plain * F_LOUD)).mean())


def _hold_automask(km, rp, ident, noise, N, tag):
    """the kernel's automask bits against the free-running oracle's: a handful of pixels apart, every one a near-tie"""
    rp, idn = np.asarray(rp), (torch.as_tensor(ident) + torch.as_tensor(noise) * 0.00001).numpy()
    d = km != _mask(rp, ident, noise)
    assert d.sum() <= 3e-4 * N + 8, (tag, "automask bits differing from the free-running oracle", int(d.sum()), N)
    assert (np.abs(rp - idn)[d] <= 1e-4).all(), (tag, "automask differs away from a tie", np.argwhere(d & (np.abs(rp - idn) > 1e-4))[:5].tolist())
    return int(d.sum())


# ------------------------------------------------------------------ DualRefine: dicts for any scale list / n_losses
def _units(scales, n_losses):
    return [(s, it) for s in scales if s != 1 for it in range(n_losses + 1 if s in (0, 1, 2) else 1)]


def _dr_dicts(batch, dev, pose_fn, scales, n_losses, pu, dtype=torch.float32):
    """_dr_build(_pu) plus the iterations beyond the second (their own leaves) and every lower scale's disparities (pooled
    copies of scale 0's, leaves of their own) and colours"""
    inputs, outputs, leaves = (_dr_build_pu if pu else _dr_build)(batch, dev, pose_fn, dtype)
    mv = lambda t: t.to(dtype).to(dev).contiguous()
    src = [batch["disp_teacher"], batch["disp_student"]] + [0.5 * batch["disp_teacher"] + 0.5 * batch["disp_student"]] * n_losses
    for it in range(2, n_losses + 1):
        leaves["disp_s0_it%d" % it] = mv(src[it]).clone().requires_grad_(True)
        outputs[("disp", 0, it)] = leaves["disp_s0_it%d" % it]
    for s in scales:
        if s in (0, 1):
            continue
        inputs[("color", 0, s)] = mv(torch.nn.functional.avg_pool2d(batch["color0"], 2 ** s))
        for it in range(n_losses + 1 if s == 2 else 1):
            leaves["disp_s%d_it%d" % (s, it)] = mv(torch.nn.functional.avg_pool2d(src[it], 2 ** s)).clone().requires_grad_(True)
            outputs[("disp", s, it)] = leaves["disp_s%d_it%d" % (s, it)]
    return inputs, outputs, leaves


def _dr_kw(B, H, W, scales, n_losses, **extra):
    kw = dict(height=H, width=W, batch_size=B, n_losses=n_losses, scales=list(scales))
    kw.update(extra)
    return kw


def _dr_step(batch, kw, pu, noises, pose_noise, backward=False):
    """DualRefineLossPath.loss_step with the decision planes -> (losses, {unit: planes}, grads)"""
    from mal_amd import dualrefine, layers
    inputs, outputs, gl = _dr_dicts(batch, DEV, layers.transformation_from_parameters, kw["scales"], kw["n_losses"], pu)
    lp = dualrefine.DualRefineLossPath(dualrefine.default_options(disable_pose_updates=not pu, **kw), fuse=True)
    with torch.set_grad_enabled(backward):
        got, decs = lp.loss_step(inputs, outputs, noises=[n.to(DEV) for n in noises], want_decisions=True,
                                 pose_noise=None if pose_noise is None else pose_noise.to(DEV))
        if backward:
            got["loss"].backward()
    torch.cuda.synchronize()
    grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).cpu().numpy() for k, t in gl.items()} if backward else None
    return {k: float(v.detach()) for k, v in got.items()}, {u: d.cpu() for u, d in decs.items()}, grads


def _dr_oracle_candidates(batch, kw, pu):
    """the free-running oracle's per-unit min_c r_c and identity term (neither depends on the noise)"""
    inputs, outputs, _ = _dr_dicts(batch, "cpu", O.transformation_from_parameters, kw["scales"], kw["n_losses"], pu)
    opt = O.dr_default_opt(**kw)
    with torch.no_grad():
        O.dr_generate_images_pred(opt, inputs, outputs)
        target = inputs[("color", 0, 0)]
        r = lambda p: O.compute_reprojection_loss(p, target)
        ident = torch.cat([r(inputs[("color", f, 0)]) for f in (-1, 1)], 1).min(1, keepdim=True)[0]
        cands = {u: torch.cat([r(outputs[("color", f) + u]) for f in (-1, 1)], 1) for u in _units(kw["scales"], kw["n_losses"])}
        if pu:
            O.dr_pose_update_generate_images_pred(opt, inputs, outputs)
            cands[("pose", 0)] = torch.cat([r(outputs[("color", -1, 0, 0, 1)]), r(outputs[("color", 1, 0, 0)])], 1)
    return {u: c.min(1, keepdim=True)[0].numpy() for u, c in cands.items()}, ident.numpy()


def _automask_bits(planes):
    return (((planes[0].long() >> 2) & 1) == 1)[:, None].numpy()


def _independent_entries(losses, unit, scales, n_losses):
    """the loss-dict entries that must not move when only `unit`'s noise map changes"""
    if unit[0] == "pose":
        return [k for k in losses if k not in ("loss", "reproj_loss/pose_0", "loss/pose_0_0")]
    s, it = unit
    last = (n_losses if s in (0, 2) else 0)
    keep = []
    for k in losses:
        if k == "loss" or k.startswith("loss/%d_" % s) or k in ("reproj_loss/pose_0", "loss/pose_0_0"):
            continue  # ("loss/s_*": the running loss of the scale, which includes this unit's term)
        if k == "reproj_loss/%d" % s and it == last:
            continue
        if k == "consistency_loss/%d_%d" % (s, it):
            continue
        keep.append(k)
    return keep + [k for k in ("reproj_loss/pose_0", "loss/pose_0_0") if k in losses]


DR_CASES = [(scales, nl, pu) for scales in ([0], [0, 2], [0, 1, 2, 3], [2, 3]) for nl in (1, 2) for pu in (False, True)
            if not (pu and 0 not in scales)]


@pytest.mark.parametrize("scales,n_losses,pose_update", DR_CASES,
                         ids=["s%s_n%d_%s" % ("".join(map(str, s)), n, "pu" if p else "nopu") for s, n, p in DR_CASES])
def test_dualrefine_noise_ownership(scales, n_losses, pose_update):
    """negate one unit's loud map at a time: that unit's automask bits move as the oracle's do (to within near-ties); every
    other unit's decision planes and loss entries stay bit for bit what they were"""
    B, H, W = 2, 40, 72
    N = B * H * W
    batch = make_batch(B, H, W, seed=1201)
    kw = _dr_kw(B, H, W, scales, n_losses)
    units = _units(scales, n_losses)
    keys = units + ([("pose", 0)] if pose_update else [])
    g = torch.Generator().manual_seed(1202)
    plain = {u: torch.randn(B, 1, H, W, generator=g) for u in keys}
    loud = {u: plain[u] * F_LOUD for u in keys}
    rp, ident = _dr_oracle_candidates(batch, kw, pose_update)
    for u in keys:
        assert _power(rp[u], ident, plain[u]) >= POWER, (u, _power(rp[u], ident, plain[u]))

    def run(maps):
        return _dr_step(batch, kw, pose_update, [maps[u] for u in units], maps.get(("pose", 0)))
    base_l, base_d, _ = run(loud)
    assert set(base_d) == set(keys)
    for u in keys:
        _hold_automask(_automask_bits(base_d[u]), rp[u], ident, loud[u], N, ("base", u))
    for u in keys:
        flipped = dict(loud)
        flipped[u] = -loud[u]
        got_l, got_d, _ = run(flipped)
        for v in keys:
            if v != u:
                assert torch.equal(got_d[v], base_d[v]), ("unit %s's planes moved when only %s's map changed" % (v, u))
        for k in _independent_entries(base_l, u, scales, n_losses):
            assert got_l[k] == base_l[k], ("loss entry %s moved when only %s's map changed" % (k, u), got_l[k], base_l[k])
        # the unit itself: the kernel's bits follow the oracle's under the negated map, and the negation really moved them
        km0, km1 = _automask_bits(base_d[u]), _automask_bits(got_d[u])
        _hold_automask(km1, rp[u], ident, flipped[u], N, ("negated", u))
        om0, om1 = _mask(rp[u], ident, loud[u]), _mask(rp[u], ident, flipped[u])
        assert (om0 != om1).mean() >= POWER, (u, (om0 != om1).mean())
        assert ((km0 != km1) != (om0 != om1)).sum() <= 2 * (3e-4 * N + 8), (u, int(((km0 != km1) != (om0 != om1)).sum()))


def _ms_dicts(batch, sclm):
    hi, hm, ho, hl = HH.ms_build(batch, DEV, sclm)
    ho.pop("lowest_cost")
    for f, s_ in ((-1, "m1"), (1, "p1")):
        hm[("axisangle", 0, f)] = hl["axisangle_" + s_]
        hm[("translation", 0, f)] = hl["translation_" + s_]
    return hi, hm, ho, hl


@pytest.mark.parametrize("temporal", [False, True], ids=["plain", "temporal"])
def test_multiscale_noise_ownership(temporal):
    """loss_step_multiscale at sclm = 3: scale s's map decides scale s's teacher automask and nothing else -- the other scales'
    teacher planes, every student plane and every loss entry of the other scales stay bit for bit"""
    from mal_amd import step, trainer
    B, H, W, sclm = 2, 40, 72, 3
    N = B * H * W
    batch = make_batch(B, H, W, seed=1211, with_syn=temporal)
    kw = dict(height=H, width=W, batch_size=B, sclm=sclm, distil=False, temporal=temporal)
    g = torch.Generator().manual_seed(1212)
    plain = [torch.randn(B, 1, H, W, generator=g) for _ in range(sclm + 1)]
    loud = [n * F_LOUD for n in plain]
    o = HH.ms_run_oracle(batch, kw, loud, loud, False, synth=HH.producer_of(batch))
    rp = [o["scales"][s]["t_cands"].min(1, keepdims=True) for s in range(sclm + 1)]
    ident = o["scales"][0]["ident"]
    for s in range(sclm + 1):
        assert _power(rp[s], ident, plain[s]) >= POWER, (s, _power(rp[s], ident, plain[s]))

    def run(maps):  # (with the backward: with the temporal hint the teacher's gradient pass, which exports the planes, runs there)
        hi, hm, ho, _ = _ms_dicts(batch, sclm)
        losses, mono, decs = step.loss_step_multiscale(trainer.default_options(**kw), hi, hm, ho, noises=[n.to(DEV) for n in maps],
                                                       image_synthesis=HH.producer_of(batch, DEV), want_decisions=True)
        losses["loss"].backward()
        torch.cuda.synchronize()
        return ({k: float(v.detach()) for k, v in losses.items()}, {k: float(v.detach()) for k, v in mono.items()},
                {k: [d.cpu() for d in v] for k, v in decs.items()})
    bl, bm, bd = run(loud)
    for s in range(sclm + 1):
        _hold_automask(_automask_bits(bd["dec_teacher"][s]), rp[s], ident, loud[s], N, ("base", s))
    for s in range(sclm + 1):
        maps = list(loud)
        maps[s] = -loud[s]
        gl, gm, gd = run(maps)
        for t in range(sclm + 1):
            assert torch.equal(gd["dec_student"][t], bd["dec_student"][t]), ("student planes moved", s, t)
            if t != s:
                assert torch.equal(gd["dec_teacher"][t], bd["dec_teacher"][t]), ("teacher planes of scale %d moved" % t, s)
                for k in ("reproj_loss/%d" % t, "loss/%d" % t, "smooth_loss/%d" % t):
                    assert gm[k] == bm[k], (s, k, gm[k], bm[k])
        for k, v in bl.items():
            if k.startswith("main/") or k.startswith("smooth_loss/multi") or k.startswith("consistency_loss"):
                assert gl[k] == v, (s, k, gl[k], v)  # the student's own terms read no noise
        km0, km1 = _automask_bits(bd["dec_teacher"][s]), _automask_bits(gd["dec_teacher"][s])
        _hold_automask(km1, rp[s], ident, maps[s], N, ("negated", s))
        om0, om1 = _mask(rp[s], ident, loud[s]), _mask(rp[s], ident, maps[s])
        assert (om0 != om1).mean() >= POWER
        assert ((km0 != km1) != (om0 != om1)).sum() <= 2 * (3e-4 * N + 8), (s, int(((km0 != km1) != (om0 != om1)).sum()))


# ------------------------------------------------------------------ parity at loud noise
@pytest.mark.parametrize("shape,kw", [((2, 40, 72), {}), ((2, 40, 72), {"temporal": True}), ((3, 37, 50), {})],
                         ids=["distil_b2_40x72", "temporal_b2_40x72", "distil_ragged_3x37x50"])
def test_single_scale_step_decision_exact_at_loud_noise(shape, kw):
    """step.loss_step (one map): the decision-exact method of test_gpu_decisions.py with the loud map"""
    B, H, W = shape
    b = make_batch(B, H, W, seed=1221, with_syn=bool(kw.get("temporal")))
    g = torch.Generator().manual_seed(1222)
    n0, n1 = torch.randn(B, 1, H, W, generator=g), torch.randn(B, 1, H, W, generator=g)
    (h, o), counts, report = check_step_decision_exact(b, kw, n0 * F_LOUD, n1 * F_LOUD, return_runs=True)
    power = _power(o["mono_cands"].min(1, keepdims=True), o["ident"], n0)
    assert power >= POWER, power
    print("power %.3f differing decisions %s" % (power, counts))


def test_multiscale_step_decision_exact_at_loud_noise():
    """loss_step_multiscale at sclm = 3, one loud map per scale, under the four-scale decision-exact gates"""
    B, H, W, sclm = 2, 40, 72, 3
    batch = make_batch(B, H, W, seed=1231)
    kw = dict(height=H, width=W, batch_size=B, sclm=sclm, distil=False)
    g = torch.Generator().manual_seed(1232)
    plain = [torch.randn(B, 1, H, W, generator=g) for _ in range(sclm + 1)]
    o = HH.ms_run_oracle(batch, kw, plain, plain, False)
    powers = [_power(o["scales"][s]["t_cands"].min(1, keepdims=True), o["scales"][s]["ident"], plain[s]) for s in range(sclm + 1)]
    assert min(powers) >= POWER, powers
    counts, report = check_multiscale_decision_exact(batch, kw, [n * F_LOUD for n in plain], False)
    print("power %s differing decisions %s" % (["%.3f" % p for p in powers], {k: v for k, v in counts.items() if v}))


@pytest.mark.parametrize("shape,scales", [((2, 40, 72), [0, 1, 2, 3]), ((3, 37, 50), [0])], ids=["b2_40x72_scales0123", "ragged_3x37x50"])
def test_dualrefine_step_and_operator_route_at_loud_noise(shape, scales):
    """upstream's default DualRefine configuration (scales [0,1,2,3], n_losses 1, pose updates on) with loud maps: the one-call
    step's automask bits of every unit against the free-running oracle's, its losses against the free-running oracle's, its
    gradients decision-exactly against the forced oracle; the operator route (compute_losses + compute_pose_update_losses)
    against the step"""
    from mal_amd import dualrefine, layers
    B, H, W = shape
    N = B * H * W
    batch = make_batch(B, H, W, seed=1241)
    kw = _dr_kw(B, H, W, scales, 1)
    units = _units(scales, 1)
    g = torch.Generator().manual_seed(1242)
    plain = [torch.randn(B, 1, H, W, generator=g) for _ in units]
    plain_pose = torch.randn(B, 1, H, W, generator=g)
    noises, nz_pose = [n * F_LOUD for n in plain], plain_pose * F_LOUD
    rp, ident = _dr_oracle_candidates(batch, kw, True)
    powers = {u: _power(rp[u], ident, n) for u, n in list(zip(units, plain)) + [(("pose", 0), plain_pose)]}
    assert min(powers.values()) >= POWER, powers
    got_l, decs, grads = _dr_step(batch, kw, True, noises, nz_pose, backward=True)
    counts = {u: _hold_automask(_automask_bits(decs[u]), rp[u], ident, n, N, u)
              for u, n in list(zip(units, noises)) + [(("pose", 0), nz_pose)]}
    build = lambda b, dev, pose_fn, dtype: _dr_dicts(b, dev, pose_fn, scales, 1, True, dtype)
    ref, _, _, _ = _dr_oracle_pu(batch, kw, noises, nz_pose, build=build)
    assert set(got_l) == set(ref), (sorted(got_l), sorted(ref))
    for k, v in ref.items():  # the free-running gate of the existing tests: two near-tie pixels per visited unit
        v = float(v.detach())
        assert abs(got_l[k] - v) <= 2e-4 * abs(v) + 1e-6 + 2.0 * (len(units) + 2) / N, (k, got_l[k], v)
    forced = {u: _dr_decode(decs[u]) for u in units}
    fpose = _dr_decode(decs[("pose", 0)])
    f32, g32, _, _ = _dr_oracle_pu(batch, kw, noises, nz_pose, forced=forced, forced_pose=fpose, build=build)
    _, g64, _, _ = _dr_oracle_pu(batch, kw, noises, nz_pose, forced=_to64(forced), forced_pose=_to64(fpose),
                                 dtype=torch.float64, build=build)
    leaf_values = {k: t.detach().numpy() for k, t in build(batch, "cpu", O.transformation_from_parameters, torch.float32)[2].items()}
    _dr_hold_against_forced_oracle(grads, leaf_values, f32, g32, g64, got_l)
    # the operator route with the same maps
    inputs, outputs, _ = _dr_dicts(batch, DEV, layers.transformation_from_parameters, scales, 1, True)
    lp = dualrefine.DualRefineLossPath(dualrefine.default_options(disable_pose_updates=False, **kw), fuse=True)
    lp.generate_images_pred(inputs, outputs)
    ops_l = lp.compute_losses(inputs, outputs, noises=[n.to(DEV) for n in noises])
    lp.pose_update_generate_images_pred(inputs, outputs)
    for k, v in lp.compute_pose_update_losses(inputs, outputs, noise=nz_pose.to(DEV)).items():
        ops_l[k] = ops_l[k] + v if k in ops_l else v
    torch.cuda.synchronize()
    for k, v in ops_l.items():
        v = float(v.detach())
        assert abs(got_l[k] - v) <= 2e-5 * abs(v) + 4.0 / N, (k, got_l[k], v)
    print("power %s differing automask bits %s" % ({u: "%.3f" % p for u, p in powers.items()}, counts))


# ------------------------------------------------------------------ in-kernel Philox streams across the calls of one step
@pytest.mark.parametrize("n_losses", [1, 2])
def test_dualrefine_in_kernel_noise_streams_across_scales(n_losses):
    """scales [0,1,2,3] with the pose update: call c of a step (one per visited scale) draws iteration it's map at step number
    (counter + c) * MAL_DR_MAX_ITERS + it and the pose-update pass at (seed ^ MAL_DR_POSE_NOISE_KEY, counter * MAL_DR_MAX_ITERS);
    the counter advances once per call.  Two consecutive drawing steps equal, bit for bit, the steps handed those maps, and
    no (key, step number) pair serves two units."""
    from mal_amd import _lib, config, dualrefine, layers, ops, step
    B, H, W = 2, 40, 72
    scales = [0, 1, 2, 3]
    calls = [s for s in scales if s != 1]
    units = _units(scales, n_losses)
    batch = make_batch(B, H, W, seed=1251)
    kw = _dr_kw(B, H, W, scales, n_losses)
    seed = 0x5eed0 + n_losses

    def draw(key, st):
        out = torch.empty(B, 1, H, W, device=DEV)
        _lib.check(_lib.load().mal_tiebreak_noise(C.c_uint64(key), C.c_uint64(st), B, H, W, out.data_ptr(), ops._stream()),
                   "mal_tiebreak_noise")
        return out

    def indices(c0):
        idx = {u: (seed, (c0 + calls.index(u[0])) * _lib.DR_MAX_ITERS + u[1]) for u in units}
        idx[("pose", 0)] = (seed ^ _lib.DR_POSE_NOISE_KEY, c0 * _lib.DR_MAX_ITERS)
        return idx

    old = config.noise_source, config.noise_seed
    config.noise_source, config.noise_seed = "philox", seed
    try:
        ctr = step.noise_counter(torch.device(DEV))
        seen = {}
        for rep in range(2):
            c0 = int(ctr.item())
            runs = []
            for mode in ("drawn", "handed"):
                idx = indices(c0)
                noises = pose_noise = None
                if mode == "handed":
                    noises = [draw(*idx[u]) for u in units]
                    pose_noise = draw(*idx[("pose", 0)])
                inputs, outputs, gl = _dr_dicts(batch, DEV, layers.transformation_from_parameters, scales, n_losses, True)
                lp = dualrefine.DualRefineLossPath(dualrefine.default_options(disable_pose_updates=False, **kw), fuse=True)
                got = lp.loss_step(inputs, outputs, noises=noises, pose_noise=pose_noise)
                got["loss"].backward()
                torch.cuda.synchronize()
                assert int(ctr.item()) == c0 + len(calls), (mode, int(ctr.item()), c0)  # the handed step leaves it
                runs.append(({k: float(v.detach()) for k, v in got.items()},
                             {k: t.grad.clone() for k, t in gl.items() if t.grad is not None}))
            assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
            for k, v in runs[0][1].items():
                assert torch.equal(v, runs[1][1][k]), k
            for u, pair in indices(c0).items():
                assert pair not in seen, ("(key, step number) %s serves %s and %s" % (pair, seen.get(pair), (rep, u)))
                seen[pair] = (rep, u)
            # the step really drew distinct maps for distinct units
            maps = [draw(*p) for p in indices(c0).values()]
            for i in range(len(maps)):
                for j in range(i):
                    assert not torch.equal(maps[i], maps[j])
    finally:
        config.noise_source, config.noise_seed = old


# ------------------------------------------------------------------ exact ties
def _symmetric(batch):
    """frame +1 := frame -1: the same image and the same pose (Rodrigues at a zero angle is I exactly, and the inverse of
    [I | t] is [I | -t] exactly, so T_m1 == T_p1 bit for bit)"""
    b = dict(batch)
    b["color_p1"] = batch["color_m1"].clone()
    b["axisangle_m1"] = torch.zeros_like(batch["axisangle_m1"])
    b["axisangle_p1"] = torch.zeros_like(batch["axisangle_p1"])
    b["translation_p1"] = -batch["translation_m1"]
    return b


def _winners_and_taps(planes):
    d = planes.long()
    return (d[0] & 3), bool(torch.equal(d[4], d[5]))


def test_single_scale_step_exact_candidate_ties_go_to_frame_minus_one():
    """the ManyDepth one-call step on a symmetric batch: both candidates of every pixel are equal, so frame -1 wins everywhere
    (torch.min's first index) in the teacher's and the student's pass, and frame +1's pose leaves receive exactly zero -- as
    the free-running oracle's do"""
    B, H, W = 2, 40, 72
    b = _symmetric(make_batch(B, H, W, seed=1261))
    from mal_amd import layers
    Tm = layers.transformation_from_parameters(b["axisangle_m1"], b["translation_m1"], True)
    Tp = layers.transformation_from_parameters(b["axisangle_p1"], b["translation_p1"], False)
    assert torch.equal(Tm, Tp)
    g = torch.Generator().manual_seed(1262)
    n0 = torch.randn(B, 1, H, W, generator=g)
    h = run_step_with_decisions(b, {}, n0)
    o = HH.run_oracle(b, {}, n0, n0)
    assert np.array_equal(o["mono_cands"][:, 0], o["mono_cands"][:, 1]) and np.array_equal(o["multi_cands"][:, 0], o["multi_cands"][:, 1])
    frac = {}
    for who in ("dec_teacher", "dec_student"):
        win, taps_equal = _winners_and_taps(h["maps"][who])
        frac[who] = float((win == 0).float().mean())
        assert taps_equal, (who, "the two frames' bilinear taps differ: the candidates are not the same computation")
        assert frac[who] == 1.0, (who, "frame +1 won an exact tie", 1.0 - frac[who])
    for k in ("axisangle_p1", "translation_p1"):
        assert not o["grads"][k].any(), (k, "oracle")
        assert not h["grads"][k].any(), (k, np.abs(h["grads"][k]).max())
    assert np.abs(h["grads"]["translation_m1"]).max() > 0
    print("bit-equal candidates (frame -1 wins): %s" % frac)


@pytest.mark.parametrize("scales", [[0], [0, 1, 2, 3]], ids=["scales0", "scales0123"])
def test_dualrefine_exact_candidate_ties_go_to_frame_minus_one(scales):
    """DualRefine's one-call step on a symmetric batch, frame -1 and frame +1 as distinct leaves holding equal 4x4 values:
    every unit's winner is frame -1 and frame +1's pose leaves receive exactly zero (the photometric term is their only
    consumer), as in the free-running oracle"""
    B, H, W = 2, 40, 72
    b = _symmetric(make_batch(B, H, W, seed=1271))
    kw = _dr_kw(B, H, W, scales, 1)
    units = _units(scales, 1)
    g = torch.Generator().manual_seed(1272)
    noises = [torch.randn(B, 1, H, W, generator=g) for _ in units]
    got_l, decs, grads = _dr_step(b, kw, False, noises, None, backward=True)
    frac = {}
    for u in units:
        win, taps_equal = _winners_and_taps(decs[u])
        frac[u] = float((win == 0).float().mean())
        assert taps_equal, (u, "the two frames' bilinear taps differ")
        assert frac[u] == 1.0, (u, "frame +1 won an exact tie", 1.0 - frac[u])
    inputs, outputs, leaves = _dr_dicts(b, "cpu", O.transformation_from_parameters, scales, 1, False)
    assert torch.equal(outputs[("cam_T_cam", 0, -1)], outputs[("cam_T_cam", 0, 1)])
    opt = O.dr_default_opt(**kw)
    O.dr_generate_images_pred(opt, inputs, outputs)
    O.dr_compute_losses(opt, inputs, outputs, noises=[n.clone() for n in noises])["loss"].backward()
    for k in ("axisangle_p1", "translation_p1"):
        assert leaves[k].grad is None or not leaves[k].grad.any(), (k, "oracle")
        assert not grads[k].any(), (k, np.abs(grads[k]).max())
    assert np.abs(grads["translation_m1"]).max() > 0
    print("bit-equal candidates (frame -1 wins): %s" % frac)


def _plateaus(batch):
    """disparities quantised to 1/64, the top quarter at the lowest level (a far, saturated sky) and a block at the highest"""
    b = dict(batch)
    for k in ("disp_teacher", "disp_student"):
        d = (torch.round(batch[k] * 64) / 64).clamp(1.0 / 64, 1.0)
        H, W = d.shape[-2:]
        d[..., :H // 4, :] = 1.0 / 64
        d[..., H // 2:, :W // 4] = float(d.max())
        b[k] = d.contiguous()
    return b


def _flat_share(disp):
    d = disp.numpy()
    return float(np.concatenate([(d[..., :, 1:] == d[..., :, :-1]).ravel(), (d[..., 1:, :] == d[..., :-1, :]).ravel()]).mean())


def test_single_scale_step_on_disparity_plateaus():
    """step.loss_step with plateaued disparities under the decision-exact gates: where neighbours are equal the smoothness
    sign is 0 (torch's sign(0)) and every pixel's gradient is held"""
    B, H, W = 2, 40, 72
    b = _plateaus(make_batch(B, H, W, seed=1281))
    assert min(_flat_share(b["disp_teacher"]), _flat_share(b["disp_student"])) >= 0.3
    g = torch.Generator().manual_seed(1282)
    n0, n1 = torch.randn(B, 1, H, W, generator=g), torch.randn(B, 1, H, W, generator=g)
    check_step_decision_exact(b, {}, n0, n1)


def test_multiscale_step_on_disparity_plateaus():
    B, H, W, sclm = 2, 40, 72, 3
    b = _plateaus(make_batch(B, H, W, seed=1291))
    assert _flat_share(b["disp_teacher"]) >= 0.3
    g = torch.Generator().manual_seed(1292)
    nt = [torch.randn(B, 1, H, W, generator=g) for _ in range(sclm + 1)]
    check_multiscale_decision_exact(b, dict(height=H, width=W, batch_size=B, sclm=sclm, distil=False), nt, False)


def test_dualrefine_step_on_disparity_plateaus():
    """DualRefine's one-call step (scale 0, n_losses 1, pose update on) with plateaued disparities, decision-exact: the
    per-pixel gradient maps are held at every pixel except where a neighbour is within a few ulp (none on a plateau)"""
    B, H, W = 2, 40, 72
    b = _plateaus(make_batch(B, H, W, seed=1301))
    kw = _dr_kw(B, H, W, [0], 1)
    g = torch.Generator().manual_seed(1302)
    noises = [torch.randn(B, 1, H, W, generator=g) for _ in range(2)]
    nz_pose = torch.randn(B, 1, H, W, generator=g)
    got_l, decs, grads = _dr_step(b, kw, True, noises, nz_pose, backward=True)
    forced = {u: _dr_decode(decs[u]) for u in ((0, 0), (0, 1))}
    fpose = _dr_decode(decs[("pose", 0)])
    f32, g32, _, _ = _dr_oracle_pu(b, kw, noises, nz_pose, forced=forced, forced_pose=fpose)
    _, g64, _, _ = _dr_oracle_pu(b, kw, noises, nz_pose, forced=_to64(forced), forced_pose=_to64(fpose), dtype=torch.float64)
    _dr_hold_against_forced_oracle(grads, {k: b[k].numpy() for k in HH.LEAVES}, f32, g32, g64, got_l)
