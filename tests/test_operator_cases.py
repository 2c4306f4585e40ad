"""CPU side of the operator sweep (tests/operator_checks.py, tests/test_gpu_operator_sweep.py): every case of every table is
admissible -- the float32 torch reference alone is inside the gate at its floor and inside every exemption cap --, and the
tables cover the bands where the kernels change behaviour, asserted from the shapes: grid caps on both sides, blocks per
sample of the pose reduction, strips / segments / tasks of the marching kernels, the 16-sample and 585/586 boundaries."""
import numpy as np
import pytest
import torch

from oracle import aten_restated as AR
from tests import operator_checks as X

F64, F32 = X.F64, X.F32


# ---------------------------------------------------------------- 1
@pytest.mark.parametrize("name", list(X.FLAT_N))
def test_flat_cases_are_admissible(name):
    c = X.flat_case(name)
    for lo, hi in X.DEPTH_RANGES:
        (o64, g64), (o32, g32) = (X.ref_disp_to_depth(c, dt, lo, hi) for dt in (F64, F32))
        X.admissible(o64, o32, forward=True, floor=1e-6, what=name)
        X.admissible(g64, g32, forward=True, what=name)
    (m64, gap), (m32, _) = X.ref_matching_mask(c, F64), X.ref_matching_mask(c, F32)
    X.hold_decisions(m32, m64.float(), gap, name, tie=1e-5)
    n = c["disp"].numel()
    if n >= 2:
        assert float(m64[0]) == 0.0 and float(m64[1]) == 0.0      # lowest_cost == 0 and a huge one
    if n > 100:
        assert 0.1 < float(X.ref_matching_mask(c, F64, False)[0].mean()) < 0.9


@pytest.mark.parametrize("name", list(X.PLANE_SHAPES))
def test_plane_cases_are_admissible(name):
    c = X.plane_case(name)
    (o64, g64), (o32, g32) = (X.ref_backproject(c, dt) for dt in (F64, F32))
    X.admissible(o64, o32, forward=True, floor=1e-5, what=name)
    X.admissible(g64, g32, forward=True, what=name)
    if c["K"].shape[0] > 1:
        assert not torch.equal(c["inv_K"][0], c["inv_K"][1])


def test_elementwise_tables_straddle_the_block_and_the_grid_cap():
    assert {1, 255, 257} <= set(X.FLAT_N.values())
    assert [X.ew_blocks(n, 2048)[1] for n in sorted(X.FLAT_N.values())] == [False, False, False, True]
    sizes = sorted(B * H * W for B, H, W in X.PLANE_SHAPES.values())
    assert sizes[0] == 4 and 255 in sizes and sizes[-1] > 2048 * 256 and any(256 < s < 512 for s in sizes)
    assert any(B == 3 for B, H, W in X.PLANE_SHAPES.values())


# ---------------------------------------------------------------- 2
def _own_taps(c, o32):
    """stand-in for the device's grids on the CPU: the float32 reference's"""
    B, _, H, W = c["disp"].shape
    return [AR.taps_of(o32["grid%d" % f], H, W, align_corners=c["conv"] == 0) for f in range(len(c["Ts"]))]


@pytest.mark.parametrize("name", list(X.WARP_CASES))
def test_warp_cases_are_admissible(name):
    c = X.warp_case(name)
    o32, _ = X.ref_warp(c, F32)
    taps = _own_taps(c, o32)
    (o64, g64), (o32, g32) = (X.ref_warp(c, dt, taps) for dt in (F64, F32))
    if c["behind"]:  # forward only: a third of the points behind the camera
        B, _, H, W = c["disp"].shape
        pts = X.O.backproject_depth(o64["depth"], c["inv_K"].double())
        z = (c["Ts"][0].double() @ pts)[:, 2]
        assert 0.25 <= float((z < 0).double().mean()) <= 0.42
        X.admissible({k: v for k, v in o64.items() if k.startswith("grid")}, o32, forward=True, floor=1e-5, what=name)
        return
    X.admissible({k: v for k, v in o64.items() if not k.startswith("warped")}, o32, forward=True, floor=1e-5, what=name)
    X.admissible({k: v for k, v in o64.items() if k.startswith("warped")}, o32, forward=True, what=name)
    X.admissible(g64, g32, what=name)
    for f in range(len(c["Ts"])):
        if c["need_T"][f]:
            assert not g64["g_T%d" % f][:, 3].abs().max() > 0          # the bottom row of g_T is exactly zero
    pts32 = X.O.backproject_depth(o32["depth"], c["inv_K"])
    (o64, g64), (o32, g32) = (X.ref_project(c, pts32, dt) for dt in (F64, F32))
    X.admissible(o64, o32, forward=True, floor=1e-5, what=name)
    X.admissible(g64, g32, what=name)


def test_warp_table_walks_the_pose_reduction():
    """tail_pose_block strides its blocks by 10 and unrolls by 8: bps 1, 2, 9 (one short), 10, 11 (one over), 21, 81 (a
    remainder of 1 after 8 rounds of 10); the last block ragged in all but one"""
    bps = {X.bps_of(H, W) for B, H, W, conv, Fr, o in X.WARP_CASES.values()}
    assert X.BPS_WANTED <= bps, bps
    assert X.bps_of(192, 432) == 81 and 192 * 432 == 81 * 1024
    assert sum((H * W) % 1024 != 0 for B, H, W, conv, Fr, o in X.WARP_CASES.values()) >= 7
    assert {conv for B, H, W, conv, Fr, o in X.WARP_CASES.values()} == {0, 1}
    assert {Fr for B, H, W, conv, Fr, o in X.WARP_CASES.values()} == {1, 2}
    assert X.WARP_CASES["bps10_96x100_b3_per_sample_K"][0] == 3
    need = {o.get("need_T") for B, H, W, conv, Fr, o in X.WARP_CASES.values()}
    assert (False, True) in need and (True, False) in need


# ---------------------------------------------------------------- 3
@pytest.mark.parametrize("name", list(X.GRID_CASES))
def test_grid_cases_are_admissible(name):
    c = X.grid_case(name)
    (o64, g64), (o32, g32) = (X.ref_grid_sample(c, dt) for dt in (F64, F32))
    X.admissible(o64, o32, forward=True, what=name)
    X.admissible(g64, g32, what=name)
    B, C, H, W = c["src"].shape
    if c["kind"] == "lattice":
        for ax, size in ((0, W), (1, H)):
            i = AR.unnormalize(c["grid"][..., ax], size, c["ac"])            # float32, as the kernel
            i64 = AR.unnormalize(c["grid"][..., ax].double(), size, c["ac"])
            assert torch.equal(i.double(), i64) and torch.equal(i64, i64.round())
            assert float(i64.min()) == -1 and float(i64.max()) == size
        clipped = X.lattice_clipped(c)
        assert not g64["g_grid"][clipped].abs().max() > 0 and not g32["g_grid"][clipped].abs().max() > 0
        assert float(c["cot"].abs().min()) > 0
    elif c["grid"][..., 0].numel() >= 16:  # beyond both borders
        for ax, size in ((0, W), (1, H)):
            i = AR.unnormalize(c["grid"][..., ax].double(), size, c["ac"])
            assert size == 1 or (float(i.min()) < -0.2 and float(i.max()) > size - 1 + 0.2)


def test_grid_table_covers_the_listed_bands():
    t = X.GRID_CASES.values()
    assert {C for B, C, H, W, Ho, Wo, ac, k in t} == {1, 3, 5}
    assert any(W == 1 for B, C, H, W, Ho, Wo, ac, k in t) and any(H == 1 for B, C, H, W, Ho, Wo, ac, k in t)
    assert any((Ho, Wo) == (1, 1) for B, C, H, W, Ho, Wo, ac, k in t)
    assert any(X.ew_blocks(B * Ho * Wo, 2048)[1] for B, C, H, W, Ho, Wo, ac, k in t)
    assert {ac for B, C, H, W, Ho, Wo, ac, k in t if k == "lattice"} == {True, False}
    for B, C, H, W, Ho, Wo, ac, k in t:
        if k == "lattice":
            assert {H - 1, W - 1} <= X.LATTICE_SIZES if ac else {H, W} <= X.LATTICE_SIZES


# ---------------------------------------------------------------- 4
@pytest.mark.parametrize("name", list(X.SSIM_CASES))
def test_ssim_cases_are_admissible(name):
    c = X.ssim_case(name)
    exempt = X.ssim_exempt(c)
    numel = c["x"].numel()
    if c["static"] is None:
        assert float(exempt.double().mean()) == 0.0, name          # nothing near the clamp: every gradient is compared
    else:
        y0, y1, x0, x1 = c["static"]
        assert float(X.ref_ssim(c, F64)[0]["out"][:, :, y0 + 1:y1 - 1, x0 + 1:x1 - 1].max()) <= 1e-4
    for reproj, no_ssim in ((False, False), (True, False), (True, True)):
        (o64, g64), (o32, g32) = (X.ref_ssim(c, dt, reproj, no_ssim) for dt in (F64, F32))
        X.admissible(o64, o32, forward=True, what=name)
        ex = exempt if not no_ssim else torch.zeros_like(exempt)
        X.admissible(X.masked(g64, ex), X.masked(g32, ex), what=name)
    assert numel <= 1.3e6


def test_reprojection_forward_only_case_is_admissible():
    (name, (B, C, H, W, _)), = X.REPROJ_FORWARD_ONLY.items()
    assert X.ew_blocks(B * H * W, 4096)[1]
    c = X.ssim_case(name)
    with torch.no_grad():
        o64 = X.O.compute_reprojection_loss(c["x"].double(), c["y"].double())
        o32 = X.O.compute_reprojection_loss(c["x"], c["y"])
    X.admissible(dict(out=o64), dict(out=o32), forward=True, what=name)


def test_ssim_table_covers_the_listed_bands():
    t = list(X.SSIM_CASES.values())
    assert {(H, W) for B, C, H, W, o in t} >= {(2, 2), (2, 7), (3, 3), (3, 2), (5, 130), (17, 64)}
    assert {C for B, C, H, W, o in t} == {1, 2, 3, 4}
    caps = [X.ew_blocks(B * C * H * W, 4096)[1] for B, C, H, W, o in t]
    assert any(caps) and not all(caps)
    assert any(o.get("zero_block") for B, C, H, W, o in t) and any("static" in o for B, C, H, W, o in t)


# ---------------------------------------------------------------- 5
@pytest.mark.parametrize("name", list(X.PHOTO_CASES) + list(X.PHOTO_BIG))
def test_photo_cases_are_admissible(name):
    c = X.photo_case(name)
    r64, rp64, am64, w64, margin = X.ref_photo_decisions(c, F64)
    r32, rp32, am32, w32, _ = X.ref_photo_decisions(c, F32)
    X.admissible(dict(min_reproj=rp64), dict(min_reproj=rp32), forward=True, what=name)
    if not c["flags"] & X.F_AVG:
        gap = torch.gather(r64, 1, am32) - rp64
        X.hold_decisions(am32, am64, gap, name + " argmin")
        if c["tie"] is not None:
            y0, y1, x0, x1 = c["tie"]
            assert not (am64[:, :, y0 + 1:y1 - 1, x0 + 1:x1 - 1] == 1).any()   # the first minimum wins
            assert (am64[:, :, y0 + 1:y1 - 1, x0 + 1:x1 - 1] == 0).any()
    if margin is not None:
        ext = c["ext"].double() if c["ext"] is not None else 1.0
        X.hold_decisions(w32.double(), w64, margin * ext, name + " automask")
        assert 0.02 < float((margin <= 0).double().mean()) < 0.98
    if c["pixel_only"]:
        return
    s1 = float(w64.sum())
    (o64, g64), (o32, g32) = (X.ref_photo_forced(c, dt, am64, w64, s1) for dt in (F64, F32))
    X.admissible(o64, o32, forward=True, what=name)
    X.admissible(g64, g32, what=name)


def test_photo_table_covers_strips_rows_and_decompositions():
    t = dict(X.PHOTO_CASES, **X.PHOTO_BIG)
    ws, hs = {W for B, H, W, n, f, o in t.values()}, {H for B, H, W, n, f, o in t.values()}
    assert {2, 59, 60, 61, 62, 63, 121, 125} <= ws and {2, 7, 8, 9, 17} <= hs
    assert {n for B, H, W, n, f, o in t.values()} == {1, 2, 3, 4}
    assert {B for B, H, W, n, f, o in t.values()} >= {1, 3}
    # strips: 62 columns forward, 60 backward -- both sides of both, and of their doubles
    assert {(W + 61) // 62 for W in ws} >= {1, 2, 3} and {(W + 59) // 60 for W in ws} >= {1, 2, 3}
    assert (60 + 59) // 60 == 1 and (61 + 59) // 60 == 2 and (62 + 61) // 62 == 1 and (63 + 61) // 62 == 2
    # option device_cus = 1: 4 wave slots, 4 waves each forward (16 tasks), 2 backward (8 tasks)
    B, H, W = t["cus1_rows_grow_2x40x130"][:3]
    assert X.march_tasks(B, H, W, 62, 10 ** 9)[1:] == (8, 30)             # a device with room: 8 rows, 30 tasks
    s, rows, n = X.march_tasks(B, H, W, 62, 16)
    assert 8 < rows < H and n <= 16                                    # the cap is met by growing the rows
    assert X.march_tasks(B, H, W, 60, 8) == (3, H, 6)
    B, H, W = t["cus1_rows_end_at_H_3x9x130"][:3]
    assert X.march_tasks(B, H, W, 62, 10 ** 9)[1:] == (8, 18)
    assert X.march_tasks(B, H, W, 62, 16) == (3, H, 9)                  # forward: one more row, and that is all of them
    assert X.march_tasks(B, H, W, 60, 8) == (3, H, 9)                   # backward: 9 tasks > 8 with rows at H: cannot be met
    B, H, W = X.PHOTO_BIG["pixel_route_b3_384x512_past_2048_blocks"][:3]
    assert X.ew_blocks(B * H * W, 2048) == (2048, True)                # 2 x 2048 partial sums fill the 4096 doubles
    flags = {f for B, H, W, n, f, o in t.values()}
    assert any(f & X.F_AVG for f in flags) and any(f & X.F_NO_SSIM for f in flags)
    for k in range(3):
        assert any(o.get("want", (1, 1, 1))[k] is False and n <= 2 for B, H, W, n, f, o in t.values())
    assert any(o.get("need") == (False, True) for B, H, W, n, f, o in t.values())


# ---------------------------------------------------------------- 6
@pytest.mark.parametrize("name", list(X.SMOOTH_CASES))
@pytest.mark.parametrize("normalise", [False, True], ids=["plain", "normalised"])
def test_smooth_cases_are_admissible(name, normalise):
    c = X.smooth_case(name)
    (o64, g64), (o32, g32) = (X.ref_smooth(c, dt, normalise) for dt in (F64, F32))
    X.admissible(o64, o32, forward=True, floor=1e-5, what=name)
    X.admissible(g64, g32, forward=True, what=name)
    B = c["disp"].shape[0]
    if B > 1 and not normalise:
        assert not g64["g_disp"][X.CONSTANT_SAMPLE].abs().max() > 0                # the constant sample: all ties


def test_smooth_table_covers_strips_segments_and_the_chunk_cap():
    march = [(B, H, W) for B, C, H, W in X.SMOOTH_CASES.values() if C == 3]
    assert {W for B, H, W in march} >= {2, 61, 62, 63, 124, 125} and {H for B, H, W in march} >= {2, 11, 12, 13, 25}
    assert {B for B, H, W in march} >= {1, 16, 17}
    assert {X.smooth_tasks(H, W)[0] for B, H, W in march} >= {1, 2, 3} and {X.smooth_tasks(H, W)[1] for B, H, W in march} >= {1, 2, 3}
    per = [X.smooth_tasks(H, W)[0] * X.smooth_tasks(H, W)[1] for B, H, W in march]
    assert max(per) > 64 and min(per) == 1
    assert X.smooth_tasks(265, 125) == (3, 23)
    pixel = [(B, C, H, W) for B, C, H, W in X.SMOOTH_CASES.values() if C != 3]
    assert {C for B, C, H, W in pixel} == {1, 2, 4}
    bites = [X.smooth_chunks(B, H, W) for B, C, H, W in pixel]
    assert (8, 7) in bites and any(want <= cap for want, cap in bites)
    assert X.smooth_chunks(*X.SMOOTH_REFUSED[:1], 2, 2)[1] == 0 and X.smooth_chunks(*X.SMOOTH_LAST_ACCEPTED[:1], 2, 2)[1] == 1
    assert all(SM in X.SMOOTH_CASES for SM in X.SMOOTH_PIXEL_C3)


# ---------------------------------------------------------------- 7
@pytest.mark.parametrize("name", list(X.DISTIL_CASES))
def test_distil_cases_are_admissible(name):
    c = X.distil_case(name)
    r64, r32 = X.ref_distil(c, F64), X.ref_distil(c, F32)
    assert torch.equal(r64["idx"], r32["idx"])                     # comparisons of float32 inputs: exact in either
    for k in ("g_cons", "g_dist", "g_4th"):
        assert (r64[k] is None) == (r32[k] is None)
        if r64[k] is not None:
            assert torch.equal(r64[k], r32[k].double()), (name, k)  # signs and 0 / 0.5 / 1 factors: exact
    X.admissible(dict(sums=r64["sums"], cons_target=r64["cons_target"]), dict(sums=r32["sums"], cons_target=r32["cons_target"]),
                 forward=True, what=name)
    idx = r64["idx"].reshape(-1)
    if c["ens_reproj"] is not None:
        assert int(idx[0]) == 0 and int(idx[1]) == 1                # mono == ens: mono; ens == multi: the ensemble
        assert set(idx.tolist()) == {0, 1, 2} or idx.numel() <= 4
    else:
        assert int(idx[1]) == 0 and 1 not in set(idx.tolist())
    assert float(r64["g_cons"].reshape(-1)[2]) == 0.0               # multi_depth == mono_depth: sign 0


def test_distil_table_covers_the_listed_bands():
    t = X.DISTIL_CASES.values()
    ns = sorted({B * H * W for B, H, W, f, o in t})
    assert ns[0] == 4 and 256 < ns[1] < 512 and X.ew_blocks(ns[-1], 2048)[1]
    assert {f for B, H, W, f, o in t} == {0, X.F_DUAL_DISTIL}
    for key in ("ens", "ext", "learned"):
        assert {bool(o.get(key)) for B, H, W, f, o in t} == {False, True}
    assert any(o.get("need_grad") is False for B, H, W, f, o in t) and any(o.get("want_ct") is False for B, H, W, f, o in t)


# ---------------------------------------------------------------- 8
def test_assembly_tables():
    assert {len(terms) for n, terms, a, o in X.AXPY_CASES.values()} == {1, 2, 6}
    ns = sorted({n for n, terms, a, o in X.AXPY_CASES.values()})
    assert ns[0] == 1 and 257 in ns and X.ew_blocks(ns[-1], 2048)[1]
    assert {(s, d) for n, terms, a, o in X.AXPY_CASES.values() for s, d, e in terms} == {(False, False), (False, True), (True, False), (True, True)}
    assert any(not o for n, terms, a, o in X.AXPY_CASES.values()) and any(a and o for n, terms, a, o in X.AXPY_CASES.values())
    assert [X.ew_blocks(n, 1024)[1] for n in X.SUM_N] == [False, False, False, False, True, True]
    for name in X.AXPY_CASES:
        val, bound = X.ref_axpy(X.axpy_case(name))
        assert torch.isfinite(val).all() and float(bound.min()) >= 0
    import math
    for n in X.SUM_N:  # a float32 accumulation would miss the bound: the table tests the float64 accumulator
        x = X.sum_case(n)
        exact = math.fsum(x.double().tolist())
        assert abs(float(x.double().sum()) - exact) <= X.sum_bound(x)
        if n >= 65:
            seq = np.cumsum(x.numpy(), dtype=np.float32)[-1]            # a sequential float32 accumulator
            assert abs(float(seq) - exact) > X.sum_bound(x), n


# ---------------------------------------------------------------- 9
@pytest.mark.parametrize("name", list(X.POSE_CASES))
def test_pose_cases_are_admissible(name):
    c = X.pose_case(name)
    (o64, g64), (o32, g32) = (X.ref_pose(c, dt) for dt in (F64, F32))
    X.admissible(o64, o32, forward=True, floor=1e-6, what=name)
    X.admissible(g64, g32, forward=True, floor=1e-5, what=name)
    assert float(c["aa"][0][0].abs().max()) == 0.0
    assert torch.isfinite(g64["g_aa0"]).all() if g64["g_aa0"] is not None else True
    if c["aa"][0].shape[0] > 2:
        assert abs(float(c["aa"][0][1].double().norm()) - 1e-6) < 1e-8


def test_pose_table_covers_the_listed_bands():
    t = X.POSE_CASES.values()
    assert {B for B, Fr, i, a, r in t} == {1, 65} and {Fr for B, Fr, i, a, r in t} == {1, 2}
    assert any(set(i) == {True, False} for B, Fr, i, a, r in t)
    assert any(a[f] and not r[f] for B, Fr, i, a, r in t for f in range(Fr))
    assert any(r[f] and not a[f] for B, Fr, i, a, r in t for f in range(Fr))
