"""The epipolar lookup and the pose-refinement step (mal_amd.epipolar -> csrc/mal_epipolar.hip) past their fixtures: the case
table of tests/epipolar_checks.py -- hypothesis-group and pixel-block tails, 1 to 4 levels down to a 1x1 level, odd channel
counts and heads that split a channel pair, LDS footprints on both sides of both path-choice boundaries, per-sample
intrinsics, hypotheses behind the camera, a sample that projects outside, heavy-tailed cotangents -- against the oracle in
fp64 under the gate of ``epipolar_checks.check``; every nullable cotangent and every subset of leaves; the solver's three
outcomes in one batch against ``oracle.epi_oracle.align_update_per_sample``.  tests/test_epipolar_cases.py shows on the CPU
that every case is admissible and that the table covers the bands."""
import itertools

import pytest
import torch

from oracle import epi_oracle as E
from tests import epipolar_checks as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


_REF = {}


def _ref(name):
    if name not in _REF:
        c = X.lookup_case(name)
        _REF[name] = (c,) + X.reference(c)
    return _REF[name]


def _hold_lookup(name, what):
    c, (o64, g64), (o32, g32) = _ref(name)
    out, grads = X.run_lookup(c)
    print(what, "forward", X.check(out, o64, o32, forward=True, what=what))
    print(what, "gradients", X.check(grads, g64, g32, numel=c["depth"].numel(), what=what))
    return c, out, grads


@pytest.mark.parametrize("name", list(X.LOOKUP_CASES))
def test_lookup_sweep(name):
    """forward and all five gradients under the default path choice"""
    c, out, grads = _hold_lookup(name, name)
    opts = X.LOOKUP_CASES[name][1]
    if "outside" in opts:  # every tap is padding: corr = mean |f1| (held above), and NOTHING reaches fmap2
        s = opts["outside"]
        assert torch.equal(grads["f2"][s], torch.zeros_like(grads["f2"][s]))
        assert float(grads["f2"][1 - s].abs().max()) > 0


@pytest.mark.parametrize("name", X.PLANES_CASES)
@pytest.mark.parametrize("planes", [0, 1, 2])
def test_odd_channels_and_split_heads_under_each_formulation(planes, name):
    from tests.test_gpu_schedule import get_option, set_options
    saved = get_option("epi_bwd_planes")
    try:
        set_options(epi_bwd_planes=planes)
        _hold_lookup(name, "%s planes=%d" % (name, planes))
    finally:
        set_options(epi_bwd_planes=saved)


@pytest.mark.parametrize("name", X.SUBSET_CASES, ids=["plane_path", "atomic_path"])
@pytest.mark.parametrize("term", ["corr", "ds", "max_dx"])
def test_one_cotangent_alone(term, name):
    """the other two cotangents are absent (None reaches the Functions' backward, NULL the C ABI)"""
    c = _ref(name)[0]
    (o64, g64), (o32, g32) = X.reference(c, terms=(term,))
    out, grads = X.run_lookup(c, terms=(term,))
    for k in X.LEAVES:  # a leaf the term does not depend on: None, or exact zeros
        if g64[k] is None:
            assert grads[k] is None or not grads[k].abs().max() > 0, (term, k)
    print(name, term, X.check(grads, g64, g32, numel=c["depth"].numel(), what="%s %s only" % (name, term)))


GROUPS = {"f1": ("f1",), "f2": ("f2",), "coords": ("depth", "poses", "delta")}


@pytest.mark.parametrize("name", X.SUBSET_CASES, ids=["plane_path", "atomic_path"])
def test_every_subset_of_leaves(name):
    """a leaf that asked for no gradient gets None; the others get what the all-leaves run gives -- bit for bit wherever the
    summation order is fixed (everything but the float-atomic scatters into the feature maps on the atomic path), and
    under the gate there"""
    c, (o64, g64), (o32, g32) = _ref(name)
    _, full = X.run_lookup(c)
    atomic = name == X.SUBSET_CASES[1]
    for n in (1, 2):
        for groups in itertools.combinations(GROUPS, n):
            need = tuple(k for gname in groups for k in GROUPS[gname])
            _, grads = X.run_lookup(c, need=need)
            for k in X.LEAVES:
                if k not in need:
                    assert grads[k] is None, (groups, k)
                elif atomic and k in ("f1", "f2"):
                    X.check({k: grads[k]}, {k: g64[k]}, {k: g32[k]}, what="%s %s" % (name, groups))
                else:
                    assert torch.equal(grads[k], full[k]), (groups, k)


# ---------------------------------------------------------------- the corner table
_CORNER = {}


def _corner(y):
    if y not in _CORNER:
        c = X.corner_case(y)
        _CORNER[y] = (c, X.corner_oracle(c, torch.float64)[0], X.corner_oracle(c, torch.float32)[0])
    return _CORNER[y]


@pytest.mark.parametrize("y", X.CORNER_Y)
def test_corner_table(y):
    """positions on and next to every bound of the shared corner code (csrc/mal_sample.h), placed exactly through the
    lookup's coordinate input: the forward under the sweep's gate; a hypothesis whose taps are all padding gives exactly
    mean |fmap1| and sends exactly nothing to fmap2, under each backward formulation.  Coordinate gradients are not
    compared: on a tap boundary the slope is one-sided (epipolar_checks)."""
    from tests.test_gpu_schedule import get_option, set_options
    c, o64, o32 = _corner(y)
    corr, g_all = X.run_corner(c, "w_all")
    print("corner y=%g" % y, X.check(dict(corr=corr), dict(corr=o64), dict(corr=o32), forward=True, what="corner y=%g" % y))
    want = X.mean_abs_f1(c)
    for j, x in enumerate(X.CORNER_X):
        if X.all_padding(x, y):
            assert torch.equal(corr[:, j], want), (x, y)
    assert c["pad"].all() or float(g_all.abs().max()) > 0
    saved = get_option("epi_bwd_planes")
    try:
        for planes in (0, 1, 2):
            set_options(epi_bwd_planes=planes)
            g_pad = X.run_corner(c, "w_pad")[1]
            assert torch.equal(g_pad, torch.zeros_like(g_pad)), (y, planes)
    finally:
        set_options(epi_bwd_planes=saved)


@pytest.mark.parametrize("y", X.CORNER_Y)
def test_corner_table_nan_and_inf(y):
    """x = NaN and x = +inf: all padding, as above; not held to the oracle"""
    c = X.corner_case(y, X.CORNER_WILD_X)
    assert c["pad"].all()
    corr, g_pad = X.run_corner(c, "w_pad")
    want = X.mean_abs_f1(c)
    for j in range(len(X.CORNER_WILD_X)):
        assert torch.equal(corr[:, j], want), (X.CORNER_WILD_X[j], y)
    assert torch.equal(g_pad, torch.zeros_like(g_pad))


# ---------------------------------------------------------------- pose refinement, piecewise
def _hold_solve_rows(got_o, got_g, o64, g64, rows):
    """the existing per-sample gate of the Cholesky solve (tests/test_gpu_epipolar.py): the conditioning of each 6x6 system"""
    ref = dict(g64)
    ref["H"] = 0.5 * (ref["H"] + ref["H"].transpose(1, 2))     # torch.linalg.cholesky's backward symmetrises d/dH
    for s in rows:
        up = o64["update"][s]
        assert float((got_o["update"][s] - up).abs().max()) <= 2e-3 * max(1e-3, float(up.abs().max())), s
        assert float((got_o["new"][s] - o64["new"][s]).abs().max()) <= 2e-3, s
        for k in ref:
            sc = float(ref[k][s].abs().max())
            assert float((got_g[k][s] - ref[k][s]).abs().max()) <= 2e-3 * sc + 1e-7, (k, s)


def _hold_failed_rows(got_o, got_g, poses, g_new, rows):
    """pose returned bit for bit with a zero update; g_new passed through, nothing to H / b"""
    for s in rows:
        assert torch.equal(got_o["new"][s], poses[s]) and torch.equal(got_o["update"][s], torch.zeros(6, 1)), s
        assert torch.equal(got_g["poses"][s], torch.zeros(4, 4) if g_new is None else g_new[s]), s
        assert torch.equal(got_g["H"][s], torch.zeros(6, 6)) and torch.equal(got_g["b"][s], torch.zeros(6)), s


@pytest.mark.parametrize("name", list(X.ALIGN_CASES))
@pytest.mark.parametrize("robust", [False, True], ids=["plain", "robust_pose_loss"])
def test_align_pieces_sweep(robust, name):
    B, C, h, w = X.ALIGN_CASES[name]
    i = X.align_case(name)
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g)
    f64, f32 = torch.float64, torch.float32
    # ---- depth2gradcoords: both cotangents, g_cp only, g_P2 only
    w_cp, w_P2 = rnd(B, 2, 1, 5, h, w), rnd(B, 4, h * w)
    for a, b_ in ((w_cp, w_P2), (w_cp, None), (None, w_P2)):
        (o64, g64), (o32, g32) = (X.oracle_gradcoords(i, dt, a, b_) for dt in (f64, f32))
        out, grads = X.run_gradcoords(i, a, b_)
        X.check(out, o64, o32, forward=True, what=name)
        assert torch.allclose(out["P2"], o32["P2"], rtol=1e-5, atol=1e-5)
        X.check(grads, g64, g32, numel=h * w, what="%s gradcoords" % name)
    # ---- normal equations on the same p2 / P2 (centres moved onto the robust mask's bounds)
    (p2, moved), P2 = X.on_the_robust_bounds(o32["c_p"]), o32["P2"]
    g_H, g_b = rnd(B, 6, 6), rnd(B, 6)
    full = None
    for use_weight, need in ((True, X.NEQ_LEAVES), (False, X.NEQ_LEAVES), (True, tuple(k for k in X.NEQ_LEAVES if k != "f2"))):
        (o64, g64), (o32, g32) = (X.oracle_normal_eq(i, p2, P2, dt, g_H, g_b, robust, use_weight, need) for dt in (f64, f32))
        out, grads = X.run_normal_eq(i, p2, P2, g_H, g_b, robust, use_weight, need)
        what = "%s normal_equations weight=%s need=%d" % (name, use_weight, len(need))
        print(what, X.check(out, o64, o32, forward=True, what=what))
        print(what, X.check(X.outside_mask(grads, moved), X.outside_mask(g64, moved), X.outside_mask(g32, moved), numel=h * w, what=what))
        if robust:  # one float outside the bounds: masked, so d/d p2 there is exactly zero (the centres ON the bounds sit on
            for yy, xx in X.robust_rejects(p2):  # tap boundaries, where the slope is one-sided: not compared, see outside_mask)
                assert not grads["p2"][0][..., yy, xx].abs().max() > 0, (what, yy, xx)
        if use_weight and len(need) == len(X.NEQ_LEAVES):
            full = grads
        elif use_weight:  # tgt features without a gradient: the call without the workspace; the rest is the same sweep
            assert grads["f2"] is None  # (d/d tgt_w is a float-atomic scatter: held by the gate above, not bit for bit)
            for k in need:
                assert k == "tgt_w" or torch.equal(grads[k], full[k]), k
    # ---- the solve, se3_exp and the pose product: both cotangents, g_update None, g_new None; on this step's H (plain or
    # robust) where the 2e-3 gate is a statement about the kernel (epipolar_checks.solve_admissible;
    # tests/test_epipolar_cases.py says which cases that is)
    H0, b0 = o32["H"], o32["b"]
    if not X.solve_admissible(H0):
        return
    g_new, g_up = rnd(B, 4, 4), rnd(B, 6, 1)
    for a, b_ in ((g_new, g_up), (g_new, None), (None, g_up)):
        o64, g64, branches = X.oracle_update(H0, b0, i["poses"], f64, a, b_)
        assert branches == [E.CHOLESKY] * B
        got_o, got_g = X.run_update(H0, b0, i["poses"], a, b_)
        _hold_solve_rows(got_o, got_g, o64, g64, range(B))


def test_solver_branches_in_one_batch():
    """Cholesky, LU, failure (singular) and failure (NaN) rows side by side: each row takes its own outcome -- upstream
    decides per batch (oracle.epi_oracle.direct_align_per_sample's docstring) -- and none touches its neighbours"""
    H, b, poses, want = X.crafted_systems()
    g = torch.Generator().manual_seed(6)
    g_new, g_up = torch.randn(6, 4, 4, generator=g), torch.randn(6, 6, 1, generator=g)
    o64, g64, br = X.oracle_update(H, b, poses, torch.float64, g_new, g_up)
    o32, g32, _ = X.oracle_update(H, b, poses, torch.float32, g_new, g_up)
    assert br == want
    got_o, got_g = X.run_update(H, b, poses, g_new, g_up)
    chol = [s for s, x in enumerate(want) if x == E.CHOLESKY]
    _hold_solve_rows(got_o, got_g, o64, g64, chol)
    for s, x in enumerate(want):
        if x == E.LU:  # the fp32 oracle's own distance from fp64 on this system, x 1.25 (README "Parity"); d/dH unsymmetrised
            for got, r64, r32 in ((got_o, o64, o32), (got_g, g64, g32)):
                rep = X.check({k: v[s] for k, v in got.items()}, {k: v[s] for k, v in r64.items()}, {k: v[s] for k, v in r32.items()},
                              forward=True, what="LU row")
                print("LU row: (kernel distance, gate = max(1e-4, 1.25 x fp32 oracle distance))", rep)
                print("LU row: fp32 oracle distance", {k: X.distance(r32[k][s], r64[k][s]) for k in r64})
    _hold_failed_rows(got_o, got_g, poses, g_new, [s for s, x in enumerate(want) if x == E.FAILED])
    # the healthy rows are what they are without the failing rows next to them
    keep = [s for s, x in enumerate(want) if x != E.FAILED]
    alone_o, alone_g = X.run_update(H[keep], b[keep], poses[keep], g_new[keep], g_up[keep])
    for k in got_o:
        assert torch.equal(got_o[k][keep], alone_o[k]), k
    for k in got_g:
        assert torch.equal(got_g[k][keep], alone_g[k]), k
