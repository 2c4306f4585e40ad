"""CPU side of the segmenter sweep (tests/segmenter_sweep_cases.py, tests/test_gpu_segmenter_sweep.py): every case has the
property it is in its table for, proven from the fp64 checkers (tests/msda_restated.py, tests/instances_restated.py) and from
mal_msda_plan / mal_instances_workspace_bytes, which are pure host code.  A case without its property fails here, not
silently on the device."""
import ctypes

import numpy as np
import pytest

from tests import instances_restated as IR
from tests import msda_restated as MR
from tests import segmenter_sweep_cases as G


@pytest.fixture(scope="module", autouse=True)
def lib():
    from mal_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ======================================================================================================================= MSDA
def test_plan_is_host_code_with_the_entry_points_checks(lib):
    from mal_amd import _lib, msda
    vec, rows, blocks = (ctypes.c_int(-1) for _ in range(3))
    lds = ctypes.c_size_t(0)
    ok = dict(N=1, S=4, Lq=1, M=1, D=4, L=1, P=1, aligned=1)  # the shape of tests/test_msda_host.py

    def plan(**kw):
        a = {**ok, **kw}
        return lib.mal_msda_plan(a["N"], a["S"], a["Lq"], a["M"], a["D"], a["L"], a["P"], a["aligned"], ctypes.byref(vec),
                                 ctypes.byref(rows), ctypes.byref(blocks), ctypes.byref(lds))

    assert plan() == 0 and (vec.value, rows.value, blocks.value, lds.value) == (4, 1, 1, 16)
    assert plan(aligned=0) == 0 and vec.value == 1
    # MAL_ESHAPE for exactly what the entry points refuse (the list of test_msda_host.py), and for nothing at the bounds
    for bad in (dict(L=0), dict(L=9), dict(P=0), dict(P=9), dict(L=5, P=7), dict(D=0), dict(D=65), dict(M=0), dict(N=0),
                dict(S=0), dict(Lq=0), dict(N=1 << 20, S=1 << 20), dict(N=-1), dict(Lq=1 << 30, M=2, D=2),
                dict(Lq=1 << 20, M=64, L=8, P=4)):
        assert plan(**bad) == -2, bad
    for good in (dict(L=8, P=4), dict(L=4, P=8), dict(D=64), dict(L=8, P=1), dict(N=1 << 10, S=1 << 10, M=8, D=64)):
        assert plan(**good) == 0, good
    assert lib.mal_msda_plan(1, 4, 1, 1, 4, 1, 1, 1, None, None, None, None) == 0
    # the segmenter's shape: one wave per query, 32 rows of 8 lanes; 16 KiB of LDS is never exceeded
    assert msda.plan(2, 2520, 2520, 8, 32, 3, 4) == (4, 32, 2 * 2520 * 8 // 32, 32 * 37 * 4)
    assert msda.plan(2, 2520, 2520, 8, 32, 3, 4, aligned=False) == (1, 8, 2 * 2520 * 8 // 8, 8 * 37 * 4)
    with pytest.raises(_lib.MalError):
        msda.plan(1, 4, 1, 1, 65, 1, 1)


def test_every_launch_of_family_a_follows_the_stated_limits():
    for (N, Lq, M, D, L, P, _) in G.ma_cases():
        S = MR.starts_of(MR.SWEEP_LEVELS[L])[1]
        for aligned in (True, False):
            vec, rows, blocks, lds = G.msda_plan(N, S, Lq, M, D, L, P, aligned)
            assert vec == (4 if D % 4 == 0 and aligned else 1)
            total, per_row = N * Lq * M, 3 * L * P + 1
            assert rows == min(G.MSDA_THREADS // (D // vec), G.MSDA_LDS_FLOATS // per_row, total) >= 1
            assert blocks == -(-total // rows) and lds == rows * per_row * 4 <= G.MSDA_LDS_FLOATS * 4
            assert rows * (D // vec) <= G.MSDA_THREADS  # every row of the workgroup has its lanes


def test_family_a_fills_every_band_and_the_old_tables_do_not():
    seen = {}
    for (N, Lq, M, D, L, P, _) in G.ma_cases():
        S = MR.starts_of(MR.SWEEP_LEVELS[L])[1]
        for band in G.msda_bands(N, Lq, M, D, L, P, S):
            seen.setdefault(band, (N, Lq, M, D, L, P))
    for band in G.MA_BANDS:
        assert band in seen, band
        print("%-34s first filled by N=%d Lq=%d M=%d D=%d L=%d P=%d" % ((band,) + seen[band]))
    # one case fills the bands the issue names together: one channel, LDS-bound rows, 5 lanes per row, ragged, two samples
    S = MR.starts_of(MR.SWEEP_LEVELS[8])[1]
    assert {"one_channel", "rows_by_lds", "lanes_per_row_do_not_divide_256", "ragged_last_workgroup",
            "workgroup_spans_two_samples"} <= G.msda_bands(3, 65, 3, 5, 8, 4, S)
    # what the fused route ran before: the two module fixtures, 160 rows in workgroups of 64 on the float4 path
    M, L, P = (MR.MODULE_CFG[k] for k in ("n_heads", "n_levels", "n_points"))
    S = MR.starts_of(MR.MODULE_LEVELS)[1]
    old = G.msda_bands(MR.MODULE_N, MR.MODULE_LQ, M, MR.MODULE_CFG["d_model"] // M, L, P, S)
    assert G.msda_plan(MR.MODULE_N, S, MR.MODULE_LQ, M, 16, L, P)[:3] == (4, 64, 3)
    # (80 rows per sample: the second workgroup of 64 does span both samples -- with one row count, M = 4 and float4 only)
    assert old == {"float4", "rows_by_threads", "ragged_last_workgroup", "workgroup_spans_two_samples"}
    assert 8 in MR.SWEEP_LEVELS and len(MR.SWEEP_LEVELS[8]) == 8 and (1, 6) in MR.SWEEP_LEVELS[8] and (5, 1) in MR.SWEEP_LEVELS[8]
    assert max(L * P for L, P in G.MA_LP) == 32 and max(L for L, _ in G.MA_LP) == 8 and max(P for _, P in G.MA_LP) == 8


@pytest.mark.parametrize("ref_dim", G.MA_REF_DIMS)
def test_family_a_puts_about_a_fifth_of_the_samples_outside(ref_dim):
    for (M, D) in ((8, 32), (3, 5)):
        for (L, P) in G.MA_LP:
            levels, value, start, off, lg, ref = G.ma_inputs(3, 65, M, D, L, P, ref_dim)
            out = 1.0 - G.inside_fraction(MR.locations(off, ref, levels, np.float64), levels)
            assert 0.08 <= out <= 0.4, (M, D, L, P, out)


@pytest.mark.parametrize("M,D", G.MC_MD)
@pytest.mark.parametrize("ref_dim,L,P", G.MC_CASES)
def test_family_c_is_exact(ref_dim, L, P, M, D):
    levels, value, start, off, lg, ref = G.mc_inputs(ref_dim, L, P, M, D)
    assert all(h & (h - 1) == 0 and w & (w - 1) == 0 for h, w in levels) and (L * P) & (L * P - 1) == 0
    assert np.array_equal(value, np.round(value)) and np.abs(value).max() <= 64
    assert np.array_equal(off * 4, np.round(off * 4)) and np.array_equal(ref * 32, np.round(ref * 32))
    assert ref_dim == 2 or set(np.unique(ref[..., 2:]).tolist()) <= {0.25, 0.5, 1.0, 2.0}
    assert (lg == lg[..., :1]).all()
    o64, loc64, w64 = G.fused_chain(value, levels, start, off, lg, ref, np.float64)
    o32, loc32, w32 = G.fused_chain(value, levels, start, off, lg, ref, np.float32)
    assert o32.dtype == np.float32 and (w64 == 1.0 / (L * P)).all() and (w32 == np.float32(1.0 / (L * P))).all()
    assert np.array_equal(loc32.astype(np.float64), loc64)
    assert np.array_equal(bits(o32), bits(o64.astype(np.float32))) and np.array_equal(o64.astype(np.float32).astype(np.float64), o64)
    inside = G.inside_fraction(loc64, levels)
    assert 0.05 <= inside < 1.0 and np.abs(o64).max() > 0, inside
    S = MR.starts_of(levels)[1]
    assert "workgroup_spans_two_samples" in G.msda_bands(2, 37, M, D, L, P, S)


@pytest.mark.parametrize("shape", G.MD_SHAPES, ids=str)
def test_family_d_softmax_extremes(shape):
    share = {}
    for kind in G.MD_KINDS:
        levels, value, start, off, lg, ref = G.md_inputs(shape, kind)
        with np.errstate(over="ignore", invalid="ignore"):
            w32, w64 = MR.softmax(lg, np.float32), MR.softmax(lg, np.float64)
        assert np.isfinite(w32).all() and np.isfinite(w64).all(), kind  # the max subtraction: no overflow, no NaN
        share[kind] = float((w32 == 0).mean())
        if kind == "one_minus_inf":
            assert (np.isneginf(lg).sum(-1) == 1).all() and np.isneginf(lg[0, 0, 0, 0]) and np.isneginf(lg[0, 1, 0, -1])
            assert (w32[np.isneginf(lg)] == 0).all() and (w32[~np.isneginf(lg)] > 0).all()
        if kind == "all_1e4":
            assert (w32 == np.float32(1.0 / lg.shape[-1])).all()
        if kind == "offset_1e6":
            assert lg.min() > 9e5 and (lg.max(-1) > lg.min(-1)).all()
            with np.errstate(over="ignore", invalid="ignore"):  # without the max subtraction every row is inf / inf
                assert not np.isfinite(np.exp(lg) / np.exp(lg).sum(-1, keepdims=True)).any()
    print(shape, "share of exact zeros in the fp32 softmax:", {k: round(v, 3) for k, v in share.items()})
    assert share["sigma30"] >= 0.02 and share["sigma120"] >= 0.5 and share["all_1e4"] == 0


def test_family_e_reaches_every_side_and_every_corner_pattern():
    for (M, D) in G.ME_MD:
        levels, value, start, loc, w = G.me_inputs(M, D)
        assert levels == ((1, 7), (7, 1), (1, 1), (8, 16))
        assert np.array_equal(loc * G.ME_GRID, np.round(loc * G.ME_GRID)) and np.array_equal(w * 64, np.round(w * 64))
        assert np.array_equal(value, np.round(value)) and np.abs(value).max() <= 8
        for (H, W), (sides, patterns, xs, ys) in zip(levels, G.me_census(loc, levels)):
            assert all(n >= 1 for n in sides.values()), (H, W, sides)
            assert set(patterns) == G.reachable_patterns(H, W), (H, W, patterns)
            for n, seen in ((W, xs), (H, ys)):
                grid = np.array(sorted(seen))
                assert grid[grid > -1].min() - n / G.ME_GRID <= -1  # the next value above -1: one grid step lower is outside
                assert grid[grid >= n].min() - n / G.ME_GRID < n   # and the first at or beyond n
                assert (grid >= n).any() and -0.5 in seen and n - 0.5 in seen
                if n & (n - 1) == 0:  # a power of two: the grid holds every one of the values
                    assert {-1.0, 0.0, n - 1.0, float(n), float(n // 2)} <= seen, (n, seen)
            print("level %dx%d: sides %s, %d patterns" % (H, W, sides, len(patterns)))
        c64, c32 = MR.core(value, levels, start, loc, w, np.float64), MR.core(value, levels, start, loc, w, np.float32)
        assert np.array_equal(bits(c32), bits(c64.astype(np.float32))) and np.array_equal(c64.astype(np.float32).astype(np.float64), c64)
    # the y >= -1 variant of the range test differs from the kernel's on these inputs: a sample at y = -1 exists whose x is inside
    H, W = levels[3]
    x, y = loc[0, :, 0, 3, 0, 0].astype(np.float64) * W - 0.5, loc[0, :, 0, 3, 0, 1].astype(np.float64) * H - 0.5
    assert ((y == -1) & (x > -1) & (x < W)).any()


def test_family_f_is_the_segmenters_table():
    levels, value, start, off, lg, ref = G.mf_inputs()
    assert levels == tuple((192 // s, 640 // s) for s in (8, 16, 32)) and value.shape == (2, 2520, 8, 32)
    assert off.shape == (2, 2520, 8, 3, 4, 2) and ref.shape == (2, 2520, 3, 2)
    assert max(h * w for h, w in levels) > max(h * w for c in MR.CASES.values() for h, w in c[4])


# ================================================================================================================== instances
@pytest.mark.parametrize("shape", G.IA_SHAPES, ids=lambda s: "x".join(map(str, s[:4])))
def test_family_ia_grids_routes_and_workspace(shape, lib):
    h, w, H, W, ragged, route, cropped = shape
    nblk = G.inst_blocks(h, w)
    assert nblk == -(-h * w // 256) and ((nblk > 1 and (h * w) % 256 != 0) == ragged)
    assert G.inst_route(w, W) == route and 4 * h - H == cropped and 0 <= cropped <= 3 and 0 <= 4 * w - W <= 3
    for N in (1, 3):
        assert lib.mal_instances_workspace_bytes(N, G.IA_Q, G.IA_K, h, w, H, W, G.IA_T) == G.inst_workspace(N, G.IA_Q, G.IA_T, h, w)
        logits, planes, thing = G.ia_inputs(shape[:4], N)
        assert np.array_equal(planes * 256, np.round(planes * 256)) and np.abs(planes).max() <= 16
        counts = []
        for n in range(N):
            c = IR.checker(logits[n], planes[n], H, W, G.IA_T, thing)
            assert c["margin_cut"] >= 1e-5 and c["margin_sel"] >= 1e-6
            counts.append(len(c["flat"]))
        assert (N == 1 and counts == [G.IA_T]) or (len(set(counts)) == 3 and 1 <= min(counts) and max(counts) <= G.IA_T), counts
    # the formula distinguishes the block counts: one more workgroup per slot is visible in the size at a larger topk
    assert lib.mal_instances_workspace_bytes(1, 200, 8, 17, 16, 68, 64, 128) == G.inst_workspace(1, 200, 128, 17, 16)
    assert G.inst_workspace(1, 200, 128, 17, 16) > G.inst_workspace(1, 200, 128, 16, 16)


def test_what_the_old_instance_tables_reach():
    old = sorted({h * w for (_, _, h, w, _, _, _) in IR.CASES.values()} | {1, 2, 6, 85, 48 * 160})
    assert all(hw < 256 or hw % 256 == 0 for hw in old)  # no ragged multi-block grid before this table
    assert sum(1 for s in G.IA_SHAPES if s[4]) == 6 and sum(1 for s in G.IA_SHAPES if s[5] == "dword" and s[6]) == 6


@pytest.mark.parametrize("name", G.ib_names())
def test_family_ib_selection_edges(name):
    Q, K, T, logits, planes, thing = G.ib_inputs(name)
    h, w, H, W = G.SMALL_PLANE
    kind = name.partition("@")[0]
    for n in range(2):
        c = IR.checker(logits[n], planes[n], H, W, T, thing)
        assert c["margin_sel"] >= 1e-6 and (T == Q * K or c["margin_cut"] >= 1e-5)
        if kind.startswith("all_"):
            assert T == Q * K and sorted(c["flat"].tolist()) == list(range(Q * K))
        if kind == "topk_1":
            assert T == 1 and len(c["flat"]) == 1
        if kind == "drop_first_64":
            keep = thing[c["flat_topk"] % K]
            assert not keep[:64].any() and keep[64:].all() and len(c["flat"]) == T - 64
        if kind == "alternate":
            keep = thing[c["flat_topk"] % K]
            assert keep[0::2].all() and not keep[1::2].any() and len(c["flat"]) == (T + 1) // 2
            assert not np.array_equal(c["flat_topk"], np.sort(c["flat_topk"]))  # the order is not the index order
    assert not np.array_equal(logits[0], logits[1]) or Q * K == 1


def test_family_ic_tells_the_rounded_rule_from_the_fp64_order():
    logits, planes = G.ic_inputs()
    T, K = G.IC_T, G.IC_K
    tiny = float(np.finfo(np.float32).tiny)
    for n, gap in enumerate(G.IC_GAPS):
        s64, s32 = IR.class_scores(logits[n]), IR.class_scores_fp32(logits[n])
        assert s32.dtype == np.float32 and len(np.unique(s64)) == len(s64)  # the fp64 values are all distinct
        small = s64 < 1e-30
        assert small.sum() == len(s64) - 2
        if gap < 100:   # denormals, kept: several distinct values, each shared by a run of candidates
            assert ((s32[small] > 0) & (s32[small] < tiny)).all()
            assert 3 <= len(np.unique(s32[small])) < small.sum()
        else:
            assert (s32[small] == 0).all()
        # the rounding is not a matter of the last bits of exp: four fp64 ulps either way round to the same float
        assert np.array_equal((s64 * (1 - 1e-15)).astype(np.float32), s32) and np.array_equal((s64 * (1 + 1e-15)).astype(np.float32), s32)
        by32, by64 = IR.select_fp32(logits[n], T), IR.select(s64, T)
        order = IR.select_fp32(logits[n], len(s64))
        assert np.array_equal(order[:T], by32)
        assert s32[order[T - 1]] == s32[order[T]] and s64[order[T - 1]] != s64[order[T]]  # the cut is inside a run of equals
        assert set(by32.tolist()) != set(by64.tolist())                                   # the two rules select different sets
        v = s32[by32].astype(np.float64)
        assert (np.diff(v) <= 0).all() and all(a < b for a, b, eq in zip(by32[:-1], by32[1:], np.diff(v) == 0) if eq)
        if gap < 100:  # distinct denormal values keep the order of their fp64 values
            assert (np.diff(v[2:]) < 0).sum() >= 1
            i, j = np.triu_indices(len(s64), 1)
            differ = s32[i] != s32[j]
            assert ((s32[i] > s32[j]) == (s64[i] > s64[j]))[differ].all()
        c = IR.checker(logits[n], planes[n], *G.SMALL_PLANE[2:], T, fp32_rule=True)
        assert np.array_equal(c["flat"], by32) and np.array_equal(c["cls_score"], v)
        print("gap %g: %d of %d scores are %s; rounded rule %s, fp64 order %s" % (
            gap, int(small.sum()), len(s64), "zero" if gap > 100 else "denormal", by32.tolist(), by64.tolist()))


def test_family_id_magnitudes():
    h, w, H, W = G.ID_SHAPE
    base = G.id_scaled_inputs(0)[1]
    ref = IR.upsample_x4(base[0], H, W)
    for exponent in (100, -100):
        logits, planes = G.id_scaled_inputs(exponent)
        assert np.array_equal(planes.astype(np.float64), base.astype(np.float64) * 2.0 ** exponent) and np.isfinite(planes).all()
        v = IR.upsample_x4(planes[0], H, W)
        assert np.array_equal(v > 0, ref > 0) and np.array_equal(v, ref * 2.0 ** exponent)  # the bytes do not change
        c = IR.checker(logits[0], planes[0], H, W, G.ID_T)
        count = c["masks"].reshape(len(c["flat"]), -1).sum(1)
        assert (count > 0).all()
        if exponent > 0:   # every sigmoid of a set pixel is 1: exp(-v) is zero from v = 2^86 on
            assert v[v > 0].min() >= 2.0 ** 80 and np.array_equal(c["mask_score"], count / (count + 1e-6))
        else:              # every one is 0.5 to fp64's last bits
            assert v[v > 0].max() <= 2.0 ** -90 and IR.rel_dist(c["mask_score"], 0.5 * count / (count + 1e-6)) <= 1e-15
    assert G.inst_blocks(h, w) == 2 and G.inst_route(w, W) == "dword" and 4 * h - H == 3


def test_family_id_general_seed_has_an_empty_band():
    """the band rule of test_gpu_instances.py::test_general_fp32_logits at 17x16 -> 65x64: a byte may differ from the fp64
    rule only inside the rounding band; with at most 2 pixels of the seeded input inside it the rule is byte equality"""
    logits, planes = G.id_general_inputs()
    H, W = G.ID_SHAPE[2:]
    c = IR.checker(logits[0], planes[0], H, W, G.ID_GENERAL_T)
    assert c["margin_cut"] >= 1e-5 and c["margin_sel"] >= 1e-6 and len(c["flat"]) == G.ID_GENERAL_T
    outside, differ, inside = IR.band_report(c["masks"], planes[0][c["query"]], H, W)
    print("general seed %d: %d of %d pixels inside the band" % (G.ID_GENERAL_SEED, inside, G.ID_GENERAL_T * H * W))
    assert (outside, differ) == (0, 0) and inside <= 2 and G.ID_GENERAL_T * H * W == 49920
