"""CPU side of the epipolar sweep (tests/epipolar_checks.py, tests/test_gpu_epipolar_sweep.py): the case table is
admissible -- the fp32 oracle alone stays inside the gate's floor and allowance on every case --, it covers every LDS band
on both sides of both path-choice boundaries whatever limit the device reports, and the per-sample solve restated in
oracle/epi_oracle.py takes the intended branch on each crafted system and equals upstream's per-batch ``direct_align``
where the whole batch is on the Cholesky branch."""
import numpy as np
import pytest
import torch

from oracle import epi_oracle as E
from tests import epipolar_checks as X


@pytest.mark.parametrize("name", list(X.LOOKUP_CASES))
def test_lookup_case_is_admissible(name):
    c = X.lookup_case(name)
    (o64, g64), (o32, g32) = X.reference(c)
    assert all(v.dtype == torch.float64 for v in list(o64.values()) + list(g64.values()))
    assert all(v.dtype == torch.float32 for v in list(o32.values()) + list(g32.values()))
    X.admissible(o64, o32, forward=True, what=name)
    X.admissible(g64, g32, what=name)
    # the case says something: hypotheses land inside the image (except where it is built not to)
    (B, C, h, w, r, L, heads), opts = X.LOOKUP_CASES[name]
    cc = o64["coords"]
    inside = ((cc[:, 0] >= 0) & (cc[:, 0] <= w - 1) & (cc[:, 1] >= 0) & (cc[:, 1] <= h - 1)).double().flatten(1).mean(1)
    if "outside" in opts:
        assert float(inside[opts["outside"]]) == 0.0
        assert torch.equal(g64["f2"][opts["outside"]], torch.zeros_like(g64["f2"][opts["outside"]]))
        assert torch.allclose(o64["corr"][opts["outside"]].reshape(L, heads, 2 * r + 1, h, w),
                              c["f1"][opts["outside"]].double().abs().reshape(heads, C // heads, h, w).mean(1)[None, :, None])
    elif h > 1:
        assert float(inside.min()) >= 0.3, inside
    if "behind" in opts:
        X0 = E.iproj(o64["ds"], c["K"].double())
        Z = (c["poses"].double() @ X0.reshape(B, 4, -1))[:, 2]
        assert 0.25 <= float((Z < 0).double().mean()) <= 0.45
        assert float((1.0 / Z > 100).double().mean()) > 0      # the clamp bites


@pytest.mark.parametrize("name", list(X.ALIGN_CASES))
@pytest.mark.parametrize("robust", [False, True], ids=["plain", "robust"])
def test_align_case_is_admissible(name, robust):
    B, C, h, w = X.ALIGN_CASES[name]
    i = X.align_case(name)
    g = torch.Generator().manual_seed(3)
    w_cp, w_P2 = torch.randn(B, 2, 1, 5, h, w, generator=g), torch.randn(B, 4, h * w, generator=g)
    (o64, g64), (o32, g32) = (X.oracle_gradcoords(i, dt, w_cp, w_P2) for dt in (torch.float64, torch.float32))
    X.admissible(o64, o32, forward=True, what=name)
    X.admissible(g64, g32, what=name)
    (p2, moved), P2 = X.on_the_robust_bounds(o32["c_p"]), o32["P2"]
    g_H, g_b = torch.randn(B, 6, 6, generator=g), torch.randn(B, 6, generator=g)
    (o64, g64), (o32, g32) = (X.oracle_normal_eq(i, p2, P2, dt, g_H, g_b, robust) for dt in (torch.float64, torch.float32))
    X.admissible(o64, o32, forward=True, what=name)
    X.admissible(X.outside_mask(g64, moved), X.outside_mask(g32, moved), what=name)
    # the solve piece runs on the plain H of every case but the one-pixel-high image (no y-gradient: never), and on the
    # robust H (the mask keeps the pixels 2 px inside the border only) of every case at least 17 pixels high and wide
    if h == 1:
        assert not X.solve_admissible(o32["H"])
    elif not robust or min(h, w) >= 17:
        assert X.solve_admissible(o32["H"]), torch.linalg.cond(o32["H"].double())
    if robust:
        for yy, xx in X.robust_rejects(p2):
            assert not g64["p2"][0][..., yy, xx].abs().max() > 0 and not g32["p2"][0][..., yy, xx].abs().max() > 0
    if robust and h * w >= 4:  # the bounds are inclusive: the first two moved centres count, the next two do not
        pts = p2[0, :, 0, 0].reshape(2, -1)
        hi = torch.tensor([w - 3.0, h - 3.0])[:, None]
        valid = ((pts >= 2) & (pts <= hi))[0]
        assert valid[:2].all() and not valid[2:4].any()


@pytest.mark.parametrize("y", X.CORNER_Y)
def test_corner_table_is_admissible(y):
    """the table of tests/test_gpu_epipolar_sweep.py::test_corner_table: the oracle is finite on it, its fp32 form is inside
    the gate's floor, and a hypothesis gives exactly mean |fmap1| -- and sends exactly nothing to fmap2 -- where
    ``all_padding`` says so and nowhere else"""
    c = X.corner_case(y)
    (o64, g64), (o32, g32) = (X.corner_oracle(c, dt) for dt in (torch.float64, torch.float32))
    assert torch.isfinite(o64).all() and torch.isfinite(o32).all() and torch.isfinite(g64).all()
    X.admissible(dict(corr=o64), dict(corr=o32), forward=True, what="corner y=%g" % y)
    want = X.mean_abs_f1(c)
    for j, x in enumerate(X.CORNER_X):
        for o in (o64, o32):
            assert bool(torch.equal(o[:, j], want.to(o.dtype))) == X.all_padding(x, y), (x, y)
    assert torch.equal(c["pad"], torch.tensor([X.all_padding(x, y) for x in X.CORNER_X]))
    for dt in (torch.float64, torch.float32):
        assert not X.corner_oracle(c, dt, "w_pad")[1].abs().max() > 0
        if not c["pad"].all():
            assert float(g64.abs().max()) > 0


def test_corner_table_meets_every_bound_of_the_corner_code():
    B, C, h, w = X.CORNER_SHAPE
    for vals, size in ((X.CORNER_X, w), (X.CORNER_Y, h)):
        fl = {float(np.floor(np.float32(v))) for v in vals}
        assert {-2.0, -1.0, 0.0, size - 1.0, float(size)} <= fl          # every floor around both edges
        assert any(v > size + 1 for v in vals)                          # past the clamp of the int conversion
        assert any(-1 < v < 0 for v in vals) and any(size - 1 < v < size for v in vals)  # one tap in, one out, both weighted
    assert any(v < -2 for v in X.CORNER_X)                               # below the clamp
    assert all(X.all_padding(x, 0.0) for x in X.CORNER_WILD_X)


def test_every_lds_band_is_covered():
    """the lookup's backward picks two planes / one plane / the atomic scatter by comparing lds and 2 lds with the limit the
    device reports (160 KB on gfx950; 64 KB where raising it fails), the align step's by comparing h w 8: with a case in
    every band, each formulation runs and both sides of both boundaries are touched under either limit"""
    look = {X.band_of(X.lookup_lds_bytes(h, w, L)) for (B, C, h, w, r, L, heads), _ in X.LOOKUP_CASES.values()}
    align = {X.band_of(X.align_lds_bytes(h, w)) for (B, C, h, w) in X.ALIGN_CASES.values()}
    assert look == set(range(len(X.BANDS_KB))), look
    assert align == set(range(len(X.BANDS_KB))), align
    # both channel parities in the bands where "fits twice" is decided, and an L > 1 pyramid that does not fit at all
    by_band = {}
    for (B, C, h, w, r, L, heads), _ in X.LOOKUP_CASES.values():
        by_band.setdefault(X.band_of(X.lookup_lds_bytes(h, w, L)), set()).add((C % 2, L > 1))
    assert {p for p, _ in by_band[3]} == {0, 1}
    assert any(deep for _, deep in by_band[4])
    for name in X.SUBSET_CASES + X.PLANES_CASES:
        assert name in X.LOOKUP_CASES
    (B, C, h, w, r, L, heads), _ = X.LOOKUP_CASES[X.SUBSET_CASES[0]]
    assert 2 * X.lookup_lds_bytes(h, w, L) <= 32 * 1024            # the plane path under any limit
    (B, C, h, w, r, L, heads), _ = X.LOOKUP_CASES[X.SUBSET_CASES[1]]
    assert X.lookup_lds_bytes(h, w, L) > 160 * 1024                # the atomic path under any limit


def test_hypothesis_groups_levels_and_heads_are_covered():
    shapes = [s for s, _ in X.LOOKUP_CASES.values()]
    assert {(2 * r + 1) % 3 for (B, C, h, w, r, L, heads) in shapes} == {0, 1, 2}
    assert {L for (B, C, h, w, r, L, heads) in shapes} == {1, 2, 3, 4}
    assert any((h >> (L - 1), w >> (L - 1)) == (1, 1) for (B, C, h, w, r, L, heads) in shapes)
    assert any(heads > 1 and (C // heads) % 2 == 1 and C % 2 == 0 for (B, C, h, w, r, L, heads) in shapes)   # a pair straddles
    assert any(C % 2 == 1 for (B, C, h, w, r, L, heads) in shapes)
    assert {63, 64, 65, 255, 257} <= {h * w for (B, C, h, w, r, L, heads) in shapes}


def test_crafted_systems_take_the_intended_branches():
    H, b, poses, want = X.crafted_systems()
    for dt in (torch.float32, torch.float64):
        assert [E.solve_branch(H[s].to(dt), b[s].to(dt)) for s in range(6)] == want
        new, up, branches = E.align_update_per_sample(H.to(dt), b.to(dt), poses.to(dt))
        assert branches == want and new.dtype == dt and up.dtype == dt
        for s, br in enumerate(want):
            if br == E.FAILED:
                assert torch.equal(new[s], poses[s].to(dt)) and torch.equal(up[s], torch.zeros(6, 1, dtype=dt))
            else:
                assert torch.isfinite(new[s]).all() and torch.isfinite(up[s]).all()
    assert torch.equal(H[1], H[1].T) and float(torch.linalg.eigvalsh(H[1].double()).min()) < -0.5
    assert float(torch.linalg.eigvalsh(H[1].double()).abs().min()) > 0.5
    assert float(H[3][:, 0].abs().max()) == 0.0 and float(H[3][0, :].abs().max()) == 0.0
    # the VJP of a failed row: g_new passed through, nothing to H / b
    g = torch.Generator().manual_seed(6)
    g_new, g_up = torch.randn(6, 4, 4, generator=g), torch.randn(6, 6, 1, generator=g)
    _, grads, _ = X.oracle_update(H, b, poses, torch.float64, g_new, g_up)
    for s in (3, 4):
        assert torch.equal(grads["poses"][s], g_new[s].double())
        assert not grads["H"][s].abs().max() > 0 and not grads["b"][s].abs().max() > 0
    assert float((grads["H"][1] - grads["H"][1].T).abs().max()) > 1e-3      # LU: d/dH is not symmetrised


def test_per_sample_equals_per_batch_on_the_cholesky_branch():
    """upstream decides the fall-back per batch, the kernel (and ``direct_align_per_sample``) per sample; where every sample
    is positive definite the two are the same computation: bit for bit in fp32, on the golden inputs and on the crafted
    positive definite rows"""
    from tests.test_epi_oracle import ALIGN_CASES, load_align
    for tag in ALIGN_CASES:
        for robust in (False, True):
            z, i = load_align(tag)
            c_p, P2 = E.depth2gradcoords(i["poses"], i["depth"], i["K"])
            a = (i["poses"], i["f1"], i["f2"], i["src_w"], i["tgt_w"], i["K"], c_p, P2, i["weight"])
            new, up = E.direct_align(*a, robust=robust)
            new_s, up_s, branches = E.direct_align_per_sample(*a, robust=robust, return_branches=True)
            assert branches == [E.CHOLESKY] * len(branches)
            assert np.array_equal(new.numpy(), new_s.numpy()) and np.array_equal(up.numpy(), up_s.numpy())
    H, b, poses, want = X.crafted_systems()
    rows = [s for s, br in enumerate(want) if br == E.CHOLESKY]
    up = torch.cholesky_solve(b[rows][..., None], torch.linalg.cholesky(H[rows]))
    new = torch.bmm(E.se3_exp(up), poses[rows])
    new_s, up_s, _ = E.align_update_per_sample(H[rows], b[rows], poses[rows])
    assert np.array_equal(new.numpy(), new_s.numpy()) and np.array_equal(up.numpy(), up_s.numpy())
