"""The operator-level kernels (mal_amd/ops.py -> csrc/mal_warp.hip, mal_photo.hip, mal_photo_march.hip, mal_pose.hip) past
their two fixtures: the case tables of tests/operator_checks.py -- grid caps on both sides, 1 to 81 blocks per sample of the
pose reduction, strips / segments / tasks of the marching kernels, the reflection pad's smallest planes, every nullable output
and cotangent -- against plain torch in float64 under the gate of ``epipolar_checks.check``, with the decisions of the
operators forced or bounded as the module's docstring says.  Every operator runs twice on the same inputs and must repeat
itself bit for bit.  tests/test_operator_cases.py shows on the CPU that every case is admissible and that the tables cover
the bands.  With MAL_OPERATOR_SWEEP_REPORT=<file> the worst distance / tolerance per operator and case is written there."""
import math
import os
import time

import pytest
import torch

from oracle import aten_restated as AR
from tests import operator_checks as X

pytestmark = pytest.mark.gpu
DEV, F64, F32 = X.DEV, X.F64, X.F32
REPORT, T0 = [], time.time()


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("MAL_OPERATOR_SWEEP_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("".join(REPORT) + "wall time of tests/test_gpu_operator_sweep.py: %.1f s\n" % (time.time() - T0))


def dev(t):
    if isinstance(t, (list, tuple)):
        return [dev(x) for x in t]
    return None if t is None else t.to(DEV).contiguous()


def cpu(t):
    if isinstance(t, (list, tuple)):
        return [cpu(x) for x in t]
    return None if t is None else t.detach().cpu()


def _flat(o):
    if isinstance(o, (list, tuple)):
        return [x for y in o for x in _flat(y)]
    return [o]


def twice(fn):
    """the operator on the same inputs twice: no floating-point atomics, so the same bits -> the first run's outputs on the CPU"""
    a, b = cpu(fn()), cpu(fn())
    for x, y in zip(_flat(a), _flat(b)):
        assert (x is None) == (y is None)
        if x is not None:
            iv = {torch.float32: torch.int32, torch.float64: torch.int64}.get(x.dtype)
            assert torch.equal(x.view(iv), y.view(iv)) if iv else torch.equal(x, y)
    return a


def hold(op, case, got, ref64, ref32, **kw):
    rep = X.check(got, ref64, ref32, what="%s %s" % (op, case), **kw)
    worst = max([r[0] / r[1] for r in rep.values()] or [0.0])
    REPORT.append("%-22s %-64s worst distance / tolerance %.3f\n" % (op, case, worst))
    print(op, case, " ".join("%s=%.2e/%.2e%s" % (k, r[0], r[1], (" outside %.1e of %.1e" % (r[2], r[3])) if len(r) > 2 else "")
                             for k, r in rep.items()))
    return rep


def note(op, case, text):
    REPORT.append("%-22s %-64s %s\n" % (op, case, text))


def options(**kw):
    """context manager: library options set and restored (tests/test_gpu_schedule.py's accessors)"""
    from contextlib import contextmanager
    from tests.test_gpu_schedule import get_option, set_options

    @contextmanager
    def cm():
        saved = {k: get_option(k) for k in kw}
        try:
            set_options(**kw)
            yield
        finally:
            set_options(**saved)
    return cm()


# ================================================================ 1. elementwise geometry
@pytest.mark.parametrize("name", list(X.FLAT_N))
def test_disp_to_depth_and_its_backward(name):
    from mal_amd import ops
    c = X.flat_case(name)
    d, gs, gd = dev(c["disp"]), dev(c["g_scaled"]), dev(c["g_depth"])
    for lo, hi in X.DEPTH_RANGES:
        tag = "%s %g..%g" % (name, lo, hi)
        for use in (("g_scaled", "g_depth"), ("g_scaled",), ("g_depth",)):  # each cotangent absent alone
            (o64, g64), (o32, g32) = (X.ref_disp_to_depth(c, dt, lo, hi, use) for dt in (F64, F32))
            scaled, depth, g = twice(lambda: ops.disp_to_depth(d, lo, hi) + (ops.disp_to_depth_bwd(
                d, gs if "g_scaled" in use else None, gd if "g_depth" in use else None, lo, hi),))
            hold("disp_to_depth", tag, dict(scaled=scaled, depth=depth), o64, o32, forward=True, floor=1e-6)
            hold("disp_to_depth_bwd", tag + " " + "+".join(use), dict(g_disp=g), g64, g32, forward=True)


@pytest.mark.parametrize("name", list(X.FLAT_N))
def test_matching_mask(name):
    from mal_amd import ops
    c = X.flat_case(name)
    for with_cmask in (True, False):
        m64, gap = X.ref_matching_mask(c, F64, with_cmask)
        got = twice(lambda: ops.matching_mask(dev(c["lowest"]), dev(c["mono"]), dev(c["cmask"]) if with_cmask else None))
        assert set(got.unique().tolist()) <= {0.0, 1.0}
        n = X.hold_decisions(got.double(), m64, gap, name, tie=1e-5)
        note("matching_mask", "%s cmask=%d" % (name, with_cmask), "decisions differing %d of %d (cap %.0f)" % (n, got.numel(), X.decision_cap(got.numel())))
        k = min(2, got.numel())
        assert not got[:k].abs().max() > 0                               # lowest_cost == 0 (1/0 = inf) and a huge one


@pytest.mark.parametrize("name", list(X.PLANE_SHAPES))
def test_backproject_its_backward_and_texel_packing(name):
    from mal_amd import ops, _lib
    B, H, W = X.PLANE_SHAPES[name]
    c = X.plane_case(name)
    (o64, g64), (o32, g32) = (X.ref_backproject(c, dt) for dt in (F64, F32))
    pts, g = twice(lambda: (ops.backproject(dev(c["depth"]), dev(c["inv_K"])), ops.backproject_bwd(dev(c["g_points"]), dev(c["inv_K"]), B, H, W)))
    hold("backproject", name, dict(points=pts), o64, o32, forward=True, floor=1e-5)
    hold("backproject_bwd", name, dict(g_depth=g), g64, g32, forward=True)
    assert torch.equal(pts[:, 3], torch.ones(B, H * W))
    img = dev(c["img"])

    def pack():
        ops.clear_packed_sources()
        return ops.packed_source(img)
    tex = twice(pack)
    assert tex.shape == (B, H, W, _lib.load().mal_texel_floats())
    assert torch.equal(tex[..., :3].view(torch.int32), c["img"].permute(0, 2, 3, 1).contiguous().view(torch.int32))
    note("pack_texels", name, "bit-equal")


# ================================================================ 2. project3d, warp
def _warp_fwd(c, pack, **kw):
    from mal_amd import ops
    saved = ops.pack_sources
    try:
        ops.pack_sources = pack
        ops.clear_packed_sources()
        depth, grids, warped = ops.warp_fwd(dev(c["disp"]), dev(c["K"]), dev(c["inv_K"]), dev(c["Ts"]), dev(c["srcs"]), 0.1, 100.0,
                                            1e-7, c["conv"], **kw)
        return depth, grids, warped
    finally:
        ops.pack_sources = saved


def _warp_bwd(c, pack, use, need_T):
    from mal_amd import ops
    Fr = len(c["Ts"])
    saved = ops.pack_sources
    try:
        ops.pack_sources = pack
        ops.clear_packed_sources()
        return ops.warp_bwd(dev(c["disp"]), dev(c["K"]), dev(c["inv_K"]), dev(c["Ts"]), dev(c["srcs"]),
                            dev(c["g_warped"]) if "g_warped" in use else [None] * Fr,
                            dev(c["g_grid"]) if "g_grid" in use else [None] * Fr,
                            dev(c["g_depth"]) if "g_depth" in use else None, 0.1, 100.0, 1e-7, c["conv"], list(need_T))
    finally:
        ops.pack_sources = saved


def _named(depth, grids, warped):
    out = dict(depth=depth)
    for f, (g, w) in enumerate(zip(grids, warped)):
        out["grid%d" % f], out["warped%d" % f] = g, w
    return {k: v for k, v in out.items() if v is not None}


def _grads_named(g_disp, g_T):
    out = dict(g_disp=g_disp)
    for f, g in enumerate(g_T):
        out["g_T%d" % f] = g
    return out


@pytest.mark.parametrize("name", list(X.WARP_CASES))
def test_warp_forward_and_backward(name):
    B, H, W, conv, Fr, opts = X.WARP_CASES[name]
    c = X.warp_case(name)
    got = _named(*twice(lambda: _warp_fwd(c, True)))
    planar = _named(*twice(lambda: _warp_fwd(c, False)))
    for k in got:  # texel copies of the sources: the same bits
        assert torch.equal(got[k].view(torch.int32), planar[k].view(torch.int32)), (name, k)
    taps = [AR.taps_of(got["grid%d" % f], H, W, align_corners=conv == 0) for f in range(Fr)]    # the kernel's own
    (o64, g64), (o32, g32) = (X.ref_warp(c, dt, taps) for dt in (F64, F32))
    sel = lambda d, p: {k: v for k, v in d.items() if k.startswith(p)}
    hold("warp_fwd", name + " grids", sel(got, "grid"), sel(o64, "grid"), o32, forward=True, floor=1e-5)
    if c["behind"]:
        return
    hold("warp_fwd", name + " depth", sel(got, "depth"), sel(o64, "depth"), o32, forward=True, floor=1e-6)
    hold("warp_fwd", name + " warped", sel(got, "warped"), sel(o64, "warped"), o32, forward=True)
    only_depth = twice(lambda: _warp_fwd(c, True, want_grid=False, want_warped=False))
    assert only_depth[1] == [None] * Fr and torch.equal(only_depth[0], got["depth"])
    only_warped = twice(lambda: _warp_fwd(c, True, want_depth=False, want_grid=False))
    assert only_warped[0] is None and all(torch.equal(a, got["warped%d" % f]) for f, a in enumerate(only_warped[2]))
    # backward: every cotangent; then each kind alone, and the other pose gradient
    subsets = [(("g_warped", "g_grid", "g_depth"), c["need_T"])]
    if X.bps_of(H, W) <= 11:
        subsets += [(("g_warped",), tuple(not n for n in c["need_T"])), (("g_grid",), c["need_T"]), (("g_depth",), (False,) * Fr)]
    for use, need_T in subsets:
        cc = dict(c, need_T=need_T)
        (_, g64), (_, g32) = (X.ref_warp(cc, dt, taps, use) for dt in (F64, F32))
        grads = _grads_named(*twice(lambda: _warp_bwd(cc, True, use, need_T)))
        planar = _grads_named(*twice(lambda: _warp_bwd(cc, False, use, need_T)))
        for k, v in grads.items():
            assert (v is None) == (planar[k] is None) and (v is None or torch.equal(v.view(torch.int32), planar[k].view(torch.int32))), (name, k)
        for f in range(Fr):
            if need_T[f]:
                assert torch.equal(grads["g_T%d" % f][:, 3], torch.zeros(B, 4)), (name, f)    # the bottom row: exactly zero
            else:
                assert grads["g_T%d" % f] is None
        hold("warp_bwd", "%s %s need_T=%s" % (name, "+".join(use), "".join(str(int(n)) for n in need_T)), grads, g64, g32, numel=B * H * W)


@pytest.mark.parametrize("name", list(X.WARP_CASES))
def test_project3d_and_its_backward(name):
    from mal_amd import ops
    B, H, W, conv, Fr, opts = X.WARP_CASES[name]
    c = X.warp_case(name)
    K, T = dev(c["K"]), dev(c["Ts"][0])
    depth = _warp_fwd(c, True, want_grid=False, want_warped=False)[0]
    pts = ops.backproject(depth, dev(c["inv_K"]))
    pts_c = cpu(pts)
    grid, z = twice(lambda: ops.project3d(pts, K, T, H, W, 1e-7, conv, want_z=True))
    grid_only, none = twice(lambda: ops.project3d(pts, K, T, H, W, 1e-7, conv, want_z=False))
    assert none is None and torch.equal(grid_only.view(torch.int32), grid.view(torch.int32))
    (o64, g64), (o32, g32) = (X.ref_project(c, pts_c, dt) for dt in (F64, F32))
    hold("project3d", name, dict(grid=grid, z=z), o64, o32, forward=True, floor=1e-5)
    if c["behind"]:
        assert 0.25 <= float((z < 0).float().mean()) <= 0.42
        return
    gg, gz = dev(c["g_grid"][0]), dev(c["g_z"])
    for use_gz, need_p, need_T in ((True, True, True), (False, True, False), (True, False, True)):
        (_, g64), (_, g32) = (X.ref_project(c, pts_c, dt, use_gz=use_gz) for dt in (F64, F32))
        g_pts, g_T = twice(lambda: ops.project3d_bwd(pts, K, T, gg, gz if use_gz else None, H, W, 1e-7, conv, need_points=need_p, need_T=need_T))
        assert (g_pts is None) == (not need_p) and (g_T is None) == (not need_T)
        if need_T:
            assert torch.equal(g_T[:, 3], torch.zeros(B, 4))
        ref = lambda g: dict(g_points=g["g_points"] if need_p else None, g_T=g["g_T"] if need_T else None)
        hold("project3d_bwd", "%s g_z=%d points=%d T=%d" % (name, use_gz, need_p, need_T), dict(g_points=g_pts, g_T=g_T), ref(g64), ref(g32),
             numel=B * H * W)


# ================================================================ 3. grid_sample
@pytest.mark.parametrize("name", list(X.GRID_CASES))
def test_grid_sample_and_its_backward(name):
    from mal_amd import ops, layers
    c = X.grid_case(name)
    src, grid, cot = dev(c["src"]), dev(c["grid"]), dev(c["cot"])
    out, g_grid = twice(lambda: (ops.grid_sample(src, grid, c["ac"]), ops.grid_sample_bwd(src, grid, cot, c["ac"])))
    (o64, g64), (o32, g32) = (X.ref_grid_sample(c, dt) for dt in (F64, F32))
    hold("grid_sample", name, dict(out=out), o64, o32, forward=True)
    lattice = c["kind"] == "lattice"
    hold("grid_sample_bwd", name, dict(g_grid=g_grid), g64, g32, forward=lattice)   # exact positions: every element
    if lattice:  # the clip's multiplier is zero exactly at 0 and size - 1 (and beyond), the cotangent has no zeros
        clipped = X.lattice_clipped(c)
        assert not g_grid[clipped].abs().max() > 0
        assert clipped.all() or float(g_grid[~clipped].abs().max()) > 0
    if c["grid"].numel() <= 4096:  # the autograd wiring of the module-level drop-in
        gl = grid.clone().requires_grad_(True)
        o = layers.grid_sample(src, gl, padding_mode="border", align_corners=c["ac"])
        (o * cot).sum().backward()
        assert torch.equal(cpu(o), out) and torch.equal(cpu(gl.grad), g_grid)


# ================================================================ 4. ssim, reprojection loss
@pytest.mark.parametrize("name", list(X.SSIM_CASES))
def test_ssim_and_its_backward(name):
    from mal_amd import ops, layers
    c = X.ssim_case(name)
    x, y, cot = dev(c["x"]), dev(c["y"]), dev(c["cot"])
    exempt = X.ssim_exempt(c)
    (o64, g64), (o32, g32) = (X.ref_ssim(c, dt) for dt in (F64, F32))
    out = twice(lambda: ops.ssim(x, y))
    hold("ssim", name, dict(out=out), o64, o32, forward=True)
    if c["static"] is not None:  # the identity term of a static frame
        y0, y1, x0, x1 = c["static"]
        assert float(out[:, :, y0 + 1:y1 - 1, x0 + 1:x1 - 1].max()) <= 1e-4
    for need_x, need_y in ((True, True), (True, False), (False, True)):
        gx, gy = twice(lambda: ops.ssim_bwd(x, y, cot, need_x=need_x, need_y=need_y))
        assert (gx is None) == (not need_x) and (gy is None) == (not need_y)
        pick = lambda g: X.masked(dict(g_x=g["g_x"] if need_x else None, g_y=g["g_y"] if need_y else None), exempt)
        hold("ssim_bwd", "%s x=%d y=%d" % (name, need_x, need_y), X.masked(dict(g_x=gx, g_y=gy), exempt), pick(g64), pick(g32))
    if name in X.SMALL_SSIM:
        xl, yl = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        o = layers.SSIM()(xl, yl)
        (o * cot).sum().backward()
        gx, gy = cpu(ops.ssim_bwd(x, y, cot))
        assert torch.equal(cpu(o), out) and torch.equal(cpu(xl.grad), gx) and torch.equal(cpu(yl.grad), gy)


@pytest.mark.parametrize("no_ssim", [False, True], ids=["ssim", "no_ssim"])
@pytest.mark.parametrize("name", list(X.SSIM_CASES))
def test_reprojection_loss_and_its_backward(name, no_ssim):
    from mal_amd import ops, loss_utils
    c = X.ssim_case(name)
    x, y, cot = dev(c["x"]), dev(c["y"]), dev(c["cot1"])
    exempt = X.ssim_exempt(c) if not no_ssim else torch.zeros(c["x"].shape, dtype=torch.bool)
    (o64, g64), (o32, g32) = (X.ref_ssim(c, dt, True, no_ssim) for dt in (F64, F32))
    out = twice(lambda: ops.reprojection_loss(x, y, no_ssim))
    hold("reprojection_loss", "%s no_ssim=%d" % (name, no_ssim), dict(out=out), o64, o32, forward=True)
    for need_p, need_t in ((True, True), (True, False), (False, True)):
        gp, gt = twice(lambda: ops.reprojection_loss_bwd(x, y, cot, no_ssim, need_pred=need_p, need_target=need_t))
        assert (gp is None) == (not need_p) and (gt is None) == (not need_t)
        pick = lambda g: X.masked(dict(g_x=g["g_x"] if need_p else None, g_y=g["g_y"] if need_t else None), exempt)
        hold("reprojection_loss_bwd", "%s no_ssim=%d pred=%d target=%d" % (name, no_ssim, need_p, need_t),
             X.masked(dict(g_x=gp, g_y=gt), exempt), pick(g64), pick(g32))
    if name in X.SMALL_SSIM:
        xl = x.clone().requires_grad_(True)
        o = loss_utils.compute_reprojection_loss(None, xl, y, no_ssim)
        (o * cot).sum().backward()
        assert torch.equal(cpu(o), out) and torch.equal(cpu(xl.grad), cpu(ops.reprojection_loss_bwd(x, y, cot, no_ssim)[0]))


def test_reprojection_loss_forward_past_the_grid_cap():
    from mal_amd import ops
    (name, _), = X.REPROJ_FORWARD_ONLY.items()
    c = X.ssim_case(name)
    with torch.no_grad():
        o64 = X.O.compute_reprojection_loss(c["x"].double(), c["y"].double())
        o32 = X.O.compute_reprojection_loss(c["x"], c["y"])
    x, y = dev(c["x"]), dev(c["y"])
    hold("reprojection_loss", name, dict(out=twice(lambda: ops.reprojection_loss(x, y))), dict(out=o64), dict(out=o32), forward=True)


# ================================================================ 5. photo_fwd / photo_bwd
def _photo(c, name, tag):
    """one pass over a photo case under the options in force -> the device's maps, sums and gradients (CPU)"""
    from mal_amd import ops
    tgt, cands = dev(c["target"]), dev(c["cands"])
    ident, noise, ext, scale = dev(c["ident"]), dev(c["noise"]), dev(c["ext"]), dev(c["scale"])
    fl = c["flags"]
    mn, am, wt, sums = twice(lambda: ops.photo_fwd(tgt, cands, ident, noise, ext, fl))
    if c["want"] != (True, True, True):  # an output switched off: the others keep their bits
        w_mn, w_am, w_wt = c["want"]
        p = twice(lambda: ops.photo_fwd(tgt, cands, ident, noise, ext, fl, want_min=w_mn, want_argmin=w_am, want_weight=w_wt))
        for full, part, wanted in ((mn, p[0], w_mn), (am, p[1], w_am), (wt, p[2], w_wt)):
            assert (part is None) == (not wanted) and (part is None or torch.equal(part, full))
        assert torch.equal(p[3], sums)
    r64, rp64, am64, w64, margin = X.ref_photo_decisions(c, F64)
    _, rp32, _, _, _ = X.ref_photo_decisions(c, F32)
    hold("photo_fwd", tag + " min", dict(min_reproj=mn), dict(min_reproj=rp64), dict(min_reproj=rp32), forward=True)
    am_l, n_am, n_wt = am.long(), 0, 0
    if fl & X.F_AVG:
        assert torch.equal(am, torch.full_like(am, 255))
    else:
        assert int(am.max()) < len(c["cands"])
        n_am = X.hold_decisions(am_l, am64, torch.gather(r64, 1, am_l) - rp64, tag + " argmin")
        if c["tie"] is not None:
            y0, y1, x0, x1 = c["tie"]
            assert not (am[:, :, y0 + 1:y1 - 1, x0 + 1:x1 - 1] == 1).any()           # the first minimum wins
    assert set(wt.unique().tolist()) <= {0.0, 1.0}
    if margin is not None:
        n_wt = X.hold_decisions(wt.double(), w64, margin * (c["ext"].double() if c["ext"] is not None else 1.0), tag + " automask")
    else:
        assert torch.equal(wt, c["ext"] if c["ext"] is not None else torch.ones_like(wt))
    note("photo_fwd", tag + " decisions", "argmin differing %d, weight differing %d of %d (cap %.0f)" % (n_am, n_wt, wt.numel(), X.decision_cap(wt.numel())))
    assert float(sums[1]) == float(wt.double().sum())                                # 0/1 weights: exact
    s1 = float(sums[1])
    (o64, g64), (o32, g32) = (X.ref_photo_forced(c, dt, am_l, wt, s1) for dt in (F64, F32))
    hold("photo_fwd", tag + " sum", dict(sum_rw=sums[:1]), o64, o32, forward=True)
    grads = None
    if not c["pixel_only"]:
        sums_d, am_d, wt_d = dev(sums), dev(am), dev(wt)
        grads = twice(lambda: ops.photo_bwd(tgt, cands, am_d, wt_d, scale, sums_d, fl & ~X.F_AUTOMASK, list(c["need"])))
        hold("photo_bwd", tag, {"g_cand%d" % i: g for i, g in enumerate(grads)}, g64, g32, numel=wt.numel())
    return mn, am, wt, sums, grads


@pytest.mark.parametrize("impl", [1, 0], ids=["marching", "pixel"])
@pytest.mark.parametrize("name", list(X.PHOTO_CASES))
def test_photo_forward_and_backward(name, impl):
    from mal_amd import ops
    c = X.photo_case(name)
    tag = "%s impl=%d" % (name, impl)
    with options(photo_impl=impl):
        mn, am, wt, sums, grads = _photo(c, name, tag)
        if c["flags"] & X.F_AUTOMASK:  # ident planted ON the device's minimum (no noise there): the kernel compares with <=
            ident, noise = c["ident"].clone(), None if c["noise"] is None else c["noise"].clone()
            plant = torch.zeros_like(ident, dtype=torch.bool)
            plant.view(-1)[::7] = True
            ident[plant] = mn[plant]
            if noise is not None:
                noise[plant] = 0.0
            wt2 = cpu(ops.photo_fwd(dev(c["target"]), dev(c["cands"]), dev(ident), dev(noise), dev(c["ext"]), c["flags"])[2])
            want = c["ext"][plant] if c["ext"] is not None else torch.ones_like(wt2[plant])
            assert torch.equal(wt2[plant], want), tag
        if c["cus1"]:  # a one-CU device: decompose grows the rows; maps keep their bits, sums stay inside the gate
            with options(device_cus=1):
                mn1, am1, wt1, sums1, grads1 = _photo(c, name, tag + " device_cus=1")
            assert torch.equal(mn1, mn) and torch.equal(am1, am) and torch.equal(wt1, wt) and float(sums1[1]) == float(sums[1])
            for a, b in zip(grads, grads1):
                assert torch.equal(a, b)


def test_photo_pixel_route_past_the_grid_cap():
    (name, _), = X.PHOTO_BIG.items()
    with options(photo_impl=0):
        _photo(X.photo_case(name), name, name)


# ================================================================ 6. smooth_loss
def _smooth(name, c, normalise, tag):
    from mal_amd import ops
    disp, img = dev(c["disp"]), dev(c["img"])
    (o64, g64), (o32, g32) = (X.ref_smooth(c, dt, normalise) for dt in (F64, F32))
    loss, g = twice(lambda: ops.smooth_loss(disp, img, normalise, True))
    loss_only, none = twice(lambda: ops.smooth_loss(disp, img, normalise, False))
    assert none is None
    hold("smooth_loss", tag, dict(loss=loss.reshape(1)), o64, o32, forward=True, floor=1e-5)
    hold("smooth_loss", tag + " need_grad=0", dict(loss=loss_only.reshape(1)), o64, o32, forward=True, floor=1e-5)
    hold("smooth_loss", tag + " gradient", dict(g_disp=g), g64, g32, forward=True)     # exact signs: every pixel
    B = c["disp"].shape[0]
    if B > 1 and not normalise:
        assert not g[X.CONSTANT_SAMPLE].abs().max() > 0                               # the constant sample: all ties


@pytest.mark.parametrize("normalise", [False, True], ids=["plain", "normalised"])
@pytest.mark.parametrize("name", list(X.SMOOTH_CASES))
def test_smooth_loss(name, normalise):
    c = X.smooth_case(name)
    _smooth(name, c, normalise, "%s normalise=%d" % (name, normalise))
    if name in X.SMOOTH_PIXEL_C3:
        with options(photo_impl=0):
            _smooth(name, c, normalise, "%s normalise=%d photo_impl=0" % (name, normalise))


def test_smooth_loss_refuses_a_batch_its_scratch_cannot_hold():
    """pixel route: the chunk cap (4096 - 2B)/5/B is 0 at B = 586 -- MAL_ESHAPE before any launch -- and 1 at B = 585"""
    from mal_amd import ops, _lib
    for (B, C, H, W), ok in ((X.SMOOTH_REFUSED, False), (X.SMOOTH_LAST_ACCEPTED, True)):
        g = torch.Generator().manual_seed(B)
        c = dict(disp=torch.sigmoid(torch.randn(B, 1, H, W, generator=g)), img=torch.rand(B, C, H, W, generator=g))
        if not ok:
            with pytest.raises(_lib.MalError):
                ops.smooth_loss(dev(c["disp"]), dev(c["img"]), True, True)
            continue
        for normalise in (False, True):
            (o64, g64), (o32, g32) = (X.ref_smooth(c, dt, normalise) for dt in (F64, F32))
            loss, gr = twice(lambda: ops.smooth_loss(dev(c["disp"]), dev(c["img"]), normalise, True))
            hold("smooth_loss", "b585_c1_2x2 normalise=%d" % normalise, dict(loss=loss.reshape(1)), o64, o32, forward=True, floor=1e-5)
            hold("smooth_loss", "b585_c1_2x2 normalise=%d gradient" % normalise, dict(g_disp=gr), g64, g32, forward=True)


# ================================================================ 7. distillation epilogue
@pytest.mark.parametrize("name", list(X.DISTIL_CASES))
def test_distil_epilogue(name):
    from mal_amd import ops
    c = X.distil_case(name)
    r64, r32 = X.ref_distil(c, F64), X.ref_distil(c, F32)
    a = [dev(c[k]) for k in ("multi_depth", "mono_depth", "multi_reproj", "mono_reproj", "ens_reproj", "ext")]
    sums, g_cons, g_dist, g_4th, ct = twice(lambda: ops.distil_epilogue(*a, flags=c["flags"], need_grad=c["need_grad"],
                                                                          want_cons_target=c["want_ct"], ens_depth=dev(c["ens_depth"])))
    floor = 4 * X.EPS24    # one float32 rounding per term (|a - b| m, the quotient), accumulated in float64
    hold("distil_epilogue", name + " sums", dict(sums=sums[2:4]), dict(sums=r64["sums"]), dict(sums=r32["sums"]), forward=True, floor=floor)
    assert (ct is None) == (not c["want_ct"])
    if ct is not None:
        hold("distil_epilogue", name + " cons_target", dict(ct=ct), dict(ct=r64["cons_target"]), dict(ct=r32["cons_target"]), forward=True, floor=floor)
    if not c["need_grad"]:
        assert g_cons is None and g_dist is None and g_4th is None
        return
    for k, g in (("g_cons", g_cons), ("g_dist", g_dist), ("g_4th", g_4th)):  # signs times 0 / 0.5 / 1 given the winner: exact
        assert (g is None) == (r64[k] is None), (name, k)
        if g is not None:
            assert torch.equal(g.double(), r64[k]), (name, k, int((g.double() != r64[k]).sum()))
    note("distil_epilogue", name + " gradients", "exact")


def test_distil_epilogue_argument_refusals():
    from mal_amd import ops, _lib
    c = X.distil_case("n258_learned")
    a = [dev(c[k]) for k in ("multi_depth", "mono_depth", "multi_reproj", "mono_reproj")]
    with pytest.raises(_lib.MalError):   # ens_depth without ens_reproj
        ops.distil_epilogue(*a, None, dev(c["ext"]), ens_depth=dev(c["ens_depth"]))
    with pytest.raises(_lib.MalError):   # ens_depth with flags
        ops.distil_epilogue(*a, dev(c["ens_reproj"]), dev(c["ext"]), flags=X.F_DUAL_DISTIL, ens_depth=dev(c["ens_depth"]))
    lib, p = _lib.load(), (lambda t: t.data_ptr())
    ws = ops.workspace(a[0].device, 1, 2, 129)
    sums = torch.zeros(8, dtype=F64, device=DEV)
    rc = lib.mal_distil_epilogue_learned(p(a[0]), p(a[1]), p(dev(c["ens_depth"])), p(a[2]), p(a[3]), None, None, 1, 2, 129, p(sums), None,
                                         None, None, None, p(ws), ws.numel(), ops._stream())
    with pytest.raises(_lib.MalError):   # the C entry point itself: refused before any launch
        _lib.check(rc, "mal_distil_epilogue_learned")


# ================================================================ 8. axpy_maps, finish_scalars, sum_f64
@pytest.mark.parametrize("name", list(X.AXPY_CASES))
def test_axpy_maps(name):
    from mal_amd import ops
    c = X.axpy_case(name)
    val, bound = X.ref_axpy(c)
    maps, scales, denoms = dev(c["maps"]), dev(c["scales"]), dev(c["denoms"])

    def run():
        out = dev(c["out"]).clone() if c["out"] is not None else None
        res = ops.axpy_maps(maps, scales, denoms, c["mults"], c["eps"], out=out, accumulate=c["accumulate"])
        assert out is None or res.data_ptr() == out.data_ptr()
        return res
    got = twice(run)
    d = (got.double() - val).abs()
    worst = float((d / bound.clamp_min(1e-300)).max())
    note("axpy_maps", name, "worst d/bound %.3f" % worst)
    assert bool((d <= bound).all()), (name, worst)


@pytest.mark.parametrize("n", [1, 64])
@pytest.mark.parametrize("with_den", [True, False])
def test_finish_scalars(n, with_den):
    from mal_amd import ops
    g = torch.Generator().manual_seed(n)
    num = torch.randn(n, generator=g, dtype=F64) * 1e3
    den = (1 + 100 * torch.rand(n, generator=g, dtype=F64)) if with_den else None
    eps, mult = 1e-7, 0.37
    got = twice(lambda: ops.finish_scalars(dev(num), dev(den), eps, mult))
    import numpy as np
    ref = num * float(np.float32(mult))
    if with_den:
        ref = ref / (den + float(np.float32(eps)))
    rel = float(((got.double() - ref).abs() / ref.abs()).max())
    note("finish_scalars", "n%d den=%d" % (n, with_den), "worst relative %.2e (bound %.2e)" % (rel, 2.0 ** -23))
    assert got.dtype == F32 and rel <= 2.0 ** -23                      # one rounding from float64


@pytest.mark.parametrize("n", X.SUM_N)
def test_sum_f64(n):
    from mal_amd import ops
    x = X.sum_case(n)
    got = twice(lambda: ops.sum_f64(dev(x)))
    exact, bound = math.fsum(x.double().tolist()), X.sum_bound(x)
    note("sum_f64", "n%d" % n, "d/bound %.3f" % (abs(float(got) - exact) / bound))
    assert got.dtype == F64 and abs(float(got) - exact) <= bound, (n, float(got), exact, bound)


# ================================================================ 9. pose
@pytest.mark.parametrize("name", list(X.POSE_CASES))
def test_pose_forward_and_backward(name):
    from mal_amd import ops
    B, Fr, inv, need_aa, need_tr = X.POSE_CASES[name]
    c = X.pose_case(name)
    (o64, g64), (o32, g32) = (X.ref_pose(c, dt) for dt in (F64, F32))
    aa, tr, g_T = dev(c["aa"]), dev(c["tr"]), dev(c["g_T"])
    Ts, (g_aa, g_tr) = twice(lambda: (ops.pose_fwd(aa, tr, inv), ops.pose_bwd(aa, tr, inv, g_T, need_aa, need_tr)))
    hold("pose_fwd", name, {"T%d" % f: T for f, T in enumerate(Ts)}, o64, o32, forward=True, floor=1e-6)
    grads = {}
    for f in range(Fr):
        grads["g_aa%d" % f], grads["g_tr%d" % f] = g_aa[f], g_tr[f]
        assert (g_aa[f] is None) == (not need_aa[f]) and (g_tr[f] is None) == (not need_tr[f])
    hold("pose_bwd", name, grads, g64, g32, forward=True, floor=1e-5)
