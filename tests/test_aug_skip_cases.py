"""The case table of the augmented-sample skip's sweep (tests/aug_skip_checks.py) reaches every branch of the merged launch's
bookkeeping, and the restated map from workgroup number to work (march_pair_kernel, mal_amd/csrc/mal_march.hip) is a
partition: every live task of each sub-pass run once, every dead task of the student's zero-filled once, nothing else."""
import ctypes

import numpy as np
import pytest

from tests import aug_skip_checks as A


def _decomps(c):
    return A.decompose(c.B, c.H, c.W, True, c.rows, c.rows), A.decompose(c.B, c.H, c.W, False, c.rows, c.rows)


def test_the_table_holds_the_minimum_rows():
    have = {(c.B, c.H, c.W, c.rows) for c in A.CASES}
    assert A.MINIMUM <= have, sorted(A.MINIMUM - have)
    for c in A.CASES:
        assert c.H >= 16 and c.W >= 24, c  # smaller images are another question
    assert {c.name for c in A.CASES if c.extra} >= {"b12_24x122_r8", "b8_17x61", "b64_16x61", "b1_16x24"}
    assert len({c.name for c in A.CASES}) == len(A.CASES)


def test_the_rows_are_what_the_table_says_of_them():
    d = {c.name: _decomps(c) for c in A.CASES}
    stu, ens = d["b1_16x24"]
    assert stu.strips * stu.segs == 1 and ens.strips * ens.segs == 1
    assert d["b3_16x24"][0].ntasks == 3 and d["b3_16x24"][0].per_xcd == 1
    stu, ens = d["b8_17x61"]
    assert (stu.strips, ens.strips, stu.segs, stu.rows) == (2, 1, 3, 8) and 17 - 2 * 8 == 1 and (17 * 61) % 2 == 1
    stu, ens = d["b9_16x62"]
    assert (stu.strips, ens.strips) == (2, 1) and 62 == A.CW_FWD
    stu, ens = d["b12_24x122_r8"]
    assert (stu.strips, ens.strips, stu.segs, ens.segs) == (3, 2, 3, 3)
    stu, ens = d["b12_24x122"]
    assert stu.rows == 8 and ens.rows == 8  # 108 tasks fit any device's resident round: the query picks the minimum
    assert d["b64_16x61"][0].strips * d["b64_16x61"][0].segs == 4
    assert not A.pair_qualifies(65, 16, 24) and all(A.pair_qualifies(c.B, c.H, c.W) for c in A.CASES if c.B <= 64)
    # the headline: 12 x 192 x 640 qualifies, its default rows are the measured 13 / (forward) 13
    assert A.pair_qualifies(12, 192, 640) and A.decompose(12, 192, 640, True).rows == 13


def test_the_restated_decomposition_is_the_library_s():
    """mal_march_geometry (march_decompose itself; no kernel is launched, "device_cus" stands in for the device query)"""
    from mal_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()

    def get(name):
        v = ctypes.c_int()
        assert lib.mal_get_option(name.encode(), ctypes.byref(v)) == 0
        return v.value
    saved = {n: get(n) for n in ("device_cus", "march_rows", "march_rows_fwd")}
    try:
        for cus in (A.MI355X_CUS, 1, 32):
            assert lib.mal_set_option(b"device_cus", cus) == 0
            for c in A.CASES + [A.Case("headline", 12, 192, 640, 0, False, ""), A.Case("fwd_rows", 12, 192, 640, 11, False, "")]:
                for rows, rows_fwd in ((c.rows, c.rows), (c.rows, 0), (0, c.rows)):
                    assert lib.mal_set_option(b"march_rows", rows) == 0 and lib.mal_set_option(b"march_rows_fwd", rows_fwd) == 0
                    for grad in (True, False):
                        s, g, r = (ctypes.c_int() for _ in range(3))
                        assert lib.mal_march_geometry(c.B, c.H, c.W, 2 if grad else 0, ctypes.byref(s), ctypes.byref(g),
                                                      ctypes.byref(r), None) == 0  # 2: MAL_F_GRAD
                        d = A.decompose(c.B, c.H, c.W, grad, rows, rows_fwd, cus)
                        assert (s.value, g.value, r.value) == (d.strips, d.segs, d.rows), (c.name, cus, rows, rows_fwd, grad)
    finally:
        for n, v in saved.items():
            lib.mal_set_option(n.encode(), v)


def test_patterns():
    for B in sorted({c.B for c in A.CASES}):
        p = A.patterns(B)
        assert all(len(v) == B and set(v) <= {0, 1} for v in p.values())
        assert len(set(p.values())) == len(p)
        masks = set(p.values())
        for want in ([0] * B, [1] * B, [1] + [0] * (B - 1), [0] * (B - 1) + [1], [(i + 1) % 2 for i in range(B)],
                     [1] * (B - 1) + [0]):
            assert tuple(want) in masks
        if B >= 33:
            assert tuple([1] * 32 + [0] * (B - 32)) in masks and tuple([0] * 32 + [1] * (B - 32)) in masks
        if B == 12:
            assert all(tuple([1] * k + [0] * (B - k)) in masks for k in range(13))
        if B >= 8:
            assert "bernoulli_0" in p and "bernoulli_1" in p
    assert A.patterns(12) == A.patterns(12)  # seeded


def _reached(cases):
    return set().union(*(A.case_branches(c) for c in cases))


def test_the_table_reaches_every_branch():
    assert _reached(A.CASES) >= set(A.BRANCHES), sorted(set(A.BRANCHES) - _reached(A.CASES))


def test_both_dead_epilogue_branches_run_with_a_dead_sample():
    kinds = {}
    for c in A.CASES:
        if A.pair_qualifies(c.B, c.H, c.W) and any(sum(p) for p in A.patterns(c.B).values()):
            kinds.setdefault(A.dead_epilogue_is_vector(c.H, c.W), []).append(c.name)
    assert "b8_17x61" in kinds[False] and "b9_16x62" in kinds[True], kinds
    assert A.dead_epilogue_is_vector(32, 64) and A.dead_epilogue_is_vector(40, 128)  # the two earlier shapes: vector only
    assert A.dead_epilogue_is_vector(192, 640)


def test_the_live_ballot():
    one, tiny = np.float32(1.0), np.float32(1.0) - np.float32(2.0 ** -24)
    assert tiny != one and one - tiny != 0
    all_, live = A.ballot_live([0, 1, 0.25, tiny, 1], True, 5)
    assert (all_, live) == (0b11111, 0b01101)
    all_, live = A.ballot_live([1, 0, 0.75, one - tiny, 0], False, 5)  # the weight formed on the host
    assert (all_, live) == (0b11111, 0b01101)
    all_, live = A.ballot_live([0] * 64, True, 64)
    assert all_ == A.M64 and live == A.M64
    all_, live = A.ballot_live([1] * 63 + [0], True, 64)
    assert live == 1 << 63 and A.nth_sample(live, 0) == 63 and A.nth_sample(~live & all_, 62) == 62
    with pytest.raises(AssertionError):
        A.nth_sample(0b101, 2)


def _check_all(B, stu, ens, masks):
    n = 0
    for pat in masks:
        all_, live = A.ballot_live(pat, True, B)
        for stu_first in (0, 1):
            A.check_map(all_, live, stu, ens, stu_first)
        A.check_map(all_, live, stu, None, 0)  # --no_ens
        n += 1
    return n


@pytest.mark.parametrize("c", [c for c in A.CASES if A.pair_qualifies(c.B, c.H, c.W)], ids=lambda c: c.name)
def test_the_map_is_a_partition(c):
    stu, ens = _decomps(c)
    if c.B <= 10:
        assert _check_all(c.B, stu, ens, A.all_masks(c.B)) == 2 ** c.B
    else:
        assert _check_all(c.B, stu, ens, A.patterns(c.B).values()) >= 8


@pytest.mark.parametrize("B", [33, 63, 64])
def test_the_map_is_a_partition_at_wide_masks(B):
    rng = np.random.default_rng(1000 + B)
    for i in range(200):
        p_dead = (0.5, 0.1, 0.9, 0.02)[i % 4]
        pat = (rng.random(B) < p_dead).astype(np.float32)
        per_s, per_e = 1 + i % 16, 1 + (i // 16 + 5 * i) % 16  # 1..16 each; equal, smaller and larger than the student's
        _check_all(B, A.abstract_decomp(B, per_s), A.abstract_decomp(B, per_e), [pat])


def test_the_check_notices_a_wrong_map(monkeypatch):
    """the partition check fails on the restatement with the last dead task left out"""
    stu, ens = _decomps(A.case("b8_17x61"))
    all_, live = A.ballot_live(A.patterns(8)["last"], True, 8)
    real = A.pair_workgroup
    monkeypatch.setattr(A, "pair_workgroup", lambda bid, *a, **k: None if real(bid, *a, **k) == ("zero", stu.ntasks - 1)
                        else real(bid, *a, **k))
    with pytest.raises(AssertionError):
        A.check_map(all_, live, stu, ens, 0)
