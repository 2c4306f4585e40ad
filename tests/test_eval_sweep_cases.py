"""CPU: every case of the validation-metric sweep (tests/eval_sweep_cases.py) has the property it is named for, proved from
the oracle's own numbers (tests/eval_oracle.py): what the radix select meets, which border paths of the resize are taken at
a valid point, the dense window's slot counts, the clamps, the planted thresholds; and the oracle's cr_log argument moves
rmse_log only."""
import numpy as np
import pytest

from tests import eval_oracle as EO
from tests import eval_sweep_cases as SC

A = {c.name: c for c in SC.select_cases()}


def facts(name):
    return [SC.select_facts(A[name], i) for i in range(len(A[name].gts))]


# ---------------------------------------------------------------- A: the select
def test_select_cases_resize_is_the_identity():
    for c in SC.select_cases():
        assert c.split == "other" and c.ms
        sd = SC.scaled(c)
        for i, g in enumerate(c.gts):
            assert g.shape == c.disp.shape[2:]
            ys, xs = np.nonzero(g)
            want = np.float32(1) / sd[i][ys, xs] * np.float32(c.sf)
            assert SC.raw_predictions(c, i).tobytes() == want.tobytes(), c.name


def test_a1_one_to_four_valid_points():
    f = facts("A1_n1to4")
    assert [x.n for x in f] == [1, 2, 3, 4] and [x.k1 for x in f] == [0, 0, 1, 1]
    assert A["A1_n1to4"].gts[0].shape == (6, 10)
    for x in f:
        assert x.distinct == x.n                       # no ties: the even counts need the min pass over two elements
        assert x.min_pass == (x.n % 2 == 0)


def test_a2_third_pass_decides_the_median_alone():
    f = facts("A2_low_byte")
    assert [x.n for x in f] == [60, 59]
    for x in f:
        assert np.unique(x.bits >> 8).size == 1, "the predictions no longer share their top 24 bits"
        assert x.distinct >= 8
    assert f[0].min_pass and not f[1].min_pass
    assert (A["A2_low_byte"].disp[0].reshape(-1).view(np.uint32) == np.float32(0.003).view(np.uint32) + np.arange(60)).all()


def test_a3_wide_range_of_first_pass_bins():
    c = A["A3_wide"]
    assert c.sf == 30.0
    for x in facts("A3_wide"):
        p = x.bits.view(np.float32)
        assert 0.0299 < p.min() < 0.0301 and 2200 < p.max() < 2250
        assert np.unique(x.bits >> 20).size >= 50 and (p >= 2.0).sum() >= 40
    assert [x.n % 2 for x in facts("A3_wide")] == [0, 1]


def test_a4_even_counts_on_both_sides_of_k1_plus_2():
    f = facts("A4_two_valued")
    assert len(f) == len(SC.A4_KINDS)
    for kind, x in zip(SC.A4_KINDS, f):
        assert x.n == 10 and x.k1 == 4 and x.distinct == 2, kind
        lo, hi = np.unique(x.bits)
        if kind.endswith("far"):
            assert lo >> 20 != hi >> 20, kind           # the first pass separates them
        else:
            assert lo >> 8 == hi >> 8 and lo != hi, kind  # only the third pass does
        n_lo = int((x.bits == lo).sum())
        if kind.startswith("5+5"):    # every copy of v1 at or below rank k1: the upper middle is the other value
            assert n_lo == 5 and x.v1 == lo and x.count_le == x.k1 + 1 and x.count_le < x.k1 + 2 and x.min_pass, kind
        elif kind.startswith("6+4"):  # six of the smaller disparity = six of the larger prediction: both middles are it
            assert n_lo == 4 and x.v1 == hi and x.count_le == 10 and x.count_le >= x.k1 + 2 and not x.min_pass, kind
        else:                         # 4+6: both middles are the smaller prediction, count(<= v1) exactly k1 + 2
            assert n_lo == 6 and x.v1 == lo and x.count_le == x.k1 + 2 and not x.min_pass, kind
    # the disparities are two-valued a < b at the valid points
    c = A["A4_two_valued"]
    for i, kind in enumerate(SC.A4_KINDS):
        ys, xs = np.nonzero(c.gts[i])
        a, b = SC.A4_FAR if kind.endswith("far") else SC.A4_LOW
        assert a < b and sorted(set(c.disp[i, 0][ys, xs].tolist())) == [float(np.float32(a)), float(np.float32(b))]
        assert int((c.disp[i, 0][ys, xs] == np.float32(a)).sum()) == int(kind[0])


def test_a5_counts_around_the_workgroup():
    f = facts("A5_workgroup")
    assert [x.n for x in f] == [1023, 1024, 1025, 2049]
    assert A["A5_workgroup"].disp.shape[2:] == (36, 64)
    assert all(x.distinct > 256 for x in f)


def test_a6_every_bin_owner_finds_a_median():
    """each thread owns four consecutive bins of the first two passes: the median's bin takes every position in its owner"""
    first, second = set(), set()
    for c in SC.select_cases() + SC.resize_cases():
        for i in range(len(c.gts)):
            x = SC.select_facts(c, i)
            first.add(x.bin12 % 4)
            second.add(x.mid12 % 4)
    assert first == {0, 1, 2, 3} and second == {0, 1, 2, 3}, (first, second)


# ---------------------------------------------------------------- B: the resize borders
def test_resize_cases_sizes_and_border_paths():
    cases = SC.resize_cases()
    got = [(c.disp.shape[2:], c.gts[0].shape) for c in cases if c.split == "other"]
    assert got == [tuple(s) for s in SC.RESIZE_SIZES]
    assert [c.split for c in cases].count("eigen") == 1
    total = dict(left=0, copy=0, first_row=0, last_row=0)
    for c in cases:
        assert c.disp.shape[2] <= 24 and c.disp.shape[3] <= 64
        n = SC.oracle(c, True)[2]
        if c.split == "other":
            assert (n == c.gts[0].size).all(), c.name   # every pixel valid
        for i in range(len(c.gts)):
            hits = SC.resize_hits(c, i)
            for k in total:
                total[k] += hits[k]
            sh, sw = c.disp.shape[2:]
            if sw == 1:
                assert hits["copy"] == n[i], c.name       # every column is the copy
            if (sh, sw) == c.gts[0].shape:
                assert hits["left"] == hits["first_row"] == hits["last_row"] == 0 and hits["copy"] == sh
            if c.gts[0].shape == (sh + 1, sw + 1):
                assert min(hits.values()) > 0, (c.name, hits)
    assert min(total.values()) > 0, total
    eig = [c for c in cases if c.split == "eigen"][0]
    assert 0 < SC.oracle(eig, True)[2][0] < eig.gts[0].size


def test_resize_scale_one_and_times_four():
    rng = np.random.default_rng(0)
    src = rng.random((6, 10)).astype(np.float32)
    ys, xs = np.nonzero(np.ones((6, 10), bool))
    assert EO.resize_at(src, 10, 6, ys, xs).tobytes() == src.tobytes()
    sx, fx = EO._taps(20, 5)
    assert sorted(set(fx[sx >= 0].tolist())) == [0.125, 0.375, 0.625, 0.875]  # exactly x4: four exact weights


# ---------------------------------------------------------------- C: the dense window
def test_dense_cases_slots_counts_and_rounding():
    y0, x0, x1 = EO.CITYSCAPES_WINDOW
    rows = {344: 2, 345: 3, 346: 4, 350: 6}
    assert int(round(346 * 0.75)) == 260 and int(round(350 * 0.75)) == 262 and 350 * 0.75 == 262.5  # half to even
    for c in SC.dense_cases():
        assert c.split == "cityscapes" and c.disp.shape[2:] in SC.DENSE_DISPS
        for gt_f64 in (True, False):
            errs, ratios, counts, res = SC.oracle(c, gt_f64)
            assert np.isfinite(errs).all() and np.isfinite(ratios).all()
            for i, (h, w, m) in enumerate(SC.dense_index()):
                assert c.gts[i].shape == (h, w)
                win, _, _, mask = EO.valid_points(SC.gts_of(c, gt_f64)[i], "cityscapes")
                slots = rows[h] * (x1 - x0)
                assert mask.shape == (rows[h], 1664) and mask.size == slots
                assert (c.gts[i][y0 + rows[h]:, x0:x1] > 0).all()      # valid depths below the kept rows: they must not count
                want = {"all": slots, "one": 1, "checker": slots // 2, "head": slots - 1024}[m]
                assert counts[i] == mask.sum() == want, (c.name, h, w, m)
                if m == "head":
                    assert not mask.reshape(-1)[:1024].any() and mask.reshape(-1)[1024:].all()
                if m == "one":
                    assert np.nonzero(mask.reshape(-1))[0][0] >= 1024
    assert {(h, w) for h, w, _ in SC.dense_index()} >= {(h, w) for h in (344, 345, 346) for w in (1857, 2048)}
    assert set(SC.DENSE_MASKS) == {"all", "one", "checker", "head"}


# ---------------------------------------------------------------- D: the options
def test_option_cases_clamp_at_both_ends():
    cases = {c.name: c for c in SC.option_cases()}
    assert (cases["D_clamps"].min_depth, cases["D_clamps"].max_depth) == (0.1, 50)
    assert cases["D_teacher_100"].disp_max == 100.0 and cases["D_teacher_100"].which == "mono"
    assert [(cases[k].ms, cases[k].sf) for k in ("D_unscaled_0.5", "D_unscaled_30")] == [(False, 0.5), (False, 30.0)]
    for gt_f64 in (True, False):
        lo, hi = SC.clamped(cases["D_clamps"], gt_f64)
        assert lo > 0 and hi > 0
        assert SC.clamped(cases["D_unscaled_0.5"], gt_f64)[0] > 0
        lo, hi = SC.clamped(cases["D_unscaled_30"], gt_f64)
        assert lo > 0 and hi > 0
        assert SC.clamped(cases["D_teacher_100"], gt_f64)[1] > 0
    # the narrower mask drops ground truth that the default one keeps
    assert (SC.oracle(cases["D_teacher_100"], True)[2] < SC.oracle(cases["D_teacher_100_default_clamps"], True)[2]).all()


# ---------------------------------------------------------------- E: placement
def test_placement_case_mixes_sizes_and_counts():
    st, mono = SC.placement_cases()
    assert len(st.gts) == len(mono.gts) == 7 and st.disp.shape == mono.disp.shape == (7, 1, 6, 10)
    assert {g.shape for g in st.gts} == {(6, 10), (7, 11), (9, 13)}
    counts = SC.oracle(st, True)[2]
    assert counts.min() == 1 and counts.max() == 117 and len(set(counts.tolist())) >= 5
    assert st.which == "student" and mono.which == "mono" and st.disp.tobytes() != mono.disp.tobytes()


# ---------------------------------------------------------------- F: compute_errors
def test_errors_sizes_cross_the_grid_stride():
    assert 262144 in SC.ERR_SIZES and 262143 in SC.ERR_SIZES and 262145 in SC.ERR_SIZES and max(SC.ERR_SIZES) > 262144 + 256
    assert min(SC.ERR_SIZES) == 1 and any(1 < n < 256 for n in SC.ERR_SIZES)
    for tag in SC.ERR_TAGS:
        g, p = SC.errors_inputs(262401, tag)
        assert (str(g.dtype), str(p.dtype)) == tuple("float" + t[1:] for t in tag.split("_"))
        head = np.array(EO.compute_errors(g[:262144], p[:262144], cr_log=True), np.float64)
        full = np.array(EO.compute_errors(g, p, cr_log=True), np.float64)
        assert (head != full).all(), tag   # the elements past the first grid stride move every metric
        assert 0 < full[4] < full[5] < full[6] < 1


def test_planted_thresholds_are_exact_and_decide_the_counts():
    for tag in SC.ERR_TAGS:
        count = {}
        for where in SC.PLACEMENTS:
            g, p = SC.threshold_inputs(tag, where)
            th = np.maximum(g / p, p / g)
            want = np.concatenate([SC.threshold_inputs(tag, where)[0][:3].astype(np.float64),
                                   SC.threshold_inputs(tag, where)[1][3:].astype(np.float64)])
            assert (th.astype(np.float64) == want).all(), (tag, where)   # the quotient is the planted value, exactly
            e = EO.compute_errors(g, p)
            count[where] = [int(round(float(e[k]) * 6)) for k in (4, 5, 6)]
        t = np.array(SC.THRESHOLDS)
        assert (t.astype(np.float32).astype(np.float64) == t).all()
        # a ratio on a threshold is not below it; one ulp under it is.  (On and one ulp above decide alike under "<":
        # the two placements differ in what a "<=" or a rounded comparison would count.)
        assert count["below"] == [2, 4, 6] and count["on"] == [0, 2, 4] and count["above"] == [0, 2, 4], (tag, count)
        g_on, g_ab = SC.threshold_inputs(tag, "on")[0], SC.threshold_inputs(tag, "above")[0]
        assert (g_ab[:3] > g_on[:3]).all()
        le = [int((np.maximum(g_ab / SC.threshold_inputs(tag, "above")[1], SC.threshold_inputs(tag, "above")[1] / g_ab) <= c).sum())
              for c in SC.THRESHOLDS]
        assert le == count["above"], tag   # "above" stays out under "<=" too, where "on" would come in


# ---------------------------------------------------------------- the oracle's cr_log argument
def test_cr_log_moves_rmse_log_only():
    moved = 0
    for c in SC.evaluator_cases():
        for gt_f64 in (True, False):
            a, ra, na, _ = SC.oracle(c, gt_f64, cr_log=True)
            b, rb, nb, _ = SC.oracle(c, gt_f64, cr_log=False)
            assert a[:, [0, 1, 2, 4, 5, 6]].tobytes() == b[:, [0, 1, 2, 4, 5, 6]].tobytes(), c.name
            assert (na == nb).all() and (ra is None) == (rb is None) and (ra is None or ra.tobytes() == rb.tobytes())
            w = np.abs(b[:, 3])
            assert (np.abs(a[:, 3] - b[:, 3]) <= 1e-6 * np.where(w > 0, w, 1) + 1e-7).all(), c.name  # a few float32 ulp of a log
            moved += int((a[:, 3] != b[:, 3]).sum())
    assert moved > 0
    for tag in SC.ERR_TAGS:
        g, p = SC.errors_inputs(1025, tag)
        a, b = EO.compute_errors(g, p, cr_log=True), EO.compute_errors(g, p)
        assert [np.asarray(v).dtype for v in a] == [np.asarray(v).dtype for v in b]
        assert [a[k] == b[k] for k in (0, 1, 2, 4, 5, 6)] == [True] * 6
        if tag == "f64_f64":
            assert a[3] == b[3]    # no float32 log in it
    # default: today's behaviour
    g, p = SC.errors_inputs(257, "f32_f32")
    assert np.array(EO.compute_errors(g, p)).tobytes() == np.array(EO.compute_errors(g, p, cr_log=False)).tobytes()
    r0 = EO.evaluate_image(A["A3_wide"].gts[0], SC.scaled(A["A3_wide"])[0], "other", True, 30.0)
    r1 = EO.evaluate_image(A["A3_wide"].gts[0], SC.scaled(A["A3_wide"])[0], "other", True, 30.0, cr_log=False)
    assert np.array(r0["errors"]).tobytes() == np.array(r1["errors"]).tobytes()
