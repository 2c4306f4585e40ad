"""march_pair_kernel's workgroup -> task map under option "side_order" 2 (tests/pair_backfill_checks.py restates it): in either
arrangement it is a partition of the live tasks of both sub-passes plus the dead tasks of the student's, and the choice
between the arrangements is taken on both sides of equality.  No GPU."""
import numpy as np
import pytest

from tests import aug_skip_checks as A
from tests import pair_backfill_checks as P

# (tasks per sample of the student's pass, of the ensemble's, of the short ensemble's): one task per sample, equal and unequal
# counts, counts that are no multiple of 8, a short decomposition equal to the long one and larger than the student's (shorter
# segments never give fewer tasks: short >= ens throughout, the grid's max() is the short one)
PER_B = [(1, 1, 1), (3, 2, 5), (4, 2, 2), (6, 6, 15), (11, 15, 24)]


def _decomps(B, per_b):
    stu, ens, short = (A.abstract_decomp(B, n) for n in per_b)
    return stu, ens, short


def _slot_choices(B, stu, ens):
    """slot counts: B for every live set, the threshold ON half the samples, one task short of all of them, A throughout"""
    per = stu.strips * stu.segs + (ens.strips * ens.segs if ens is not None else 0)
    return sorted({0, (B + 1) // 2 * per, B * per - 1, B * per})


@pytest.mark.parametrize("B", range(1, 11))
def test_partition_every_mask(B):
    seen = set()
    for per_b in (PER_B if B <= 6 else PER_B[1:4:2]):  # every mask of every B under two decompositions at least
        stu, ens, short = _decomps(B, per_b)
        for no_ens in (False, True):
            e, s = (None, None) if no_ens else (ens, short)
            for slots in _slot_choices(B, stu, e):
                for live in range(1 << B):
                    seen.add(P.check_map((1 << B) - 1, live, stu, e, s, 2, slots))
            for order in ((0, 1) if B <= 8 else ()):  # the forced arrangement: the map of tests/aug_skip_checks.py, workgroup for workgroup
                for live in range(1 << B):
                    assert not P.check_map((1 << B) - 1, live, stu, e, s, order, 0)
                    for bid in range(P.pair_grid(stu, e, s)):
                        old = A.pair_workgroup(bid, (1 << B) - 1, live, stu, e, order) if bid < sum(A.pair_grid(stu, e)) else None
                        assert P.pair_workgroup(bid, (1 << B) - 1, live, stu, e, s, order, 0) == old
    assert seen == {False, True}


@pytest.mark.parametrize("B", [33, 63, 64])
def test_partition_seeded_masks(B):
    rng = np.random.default_rng(0xb0 + B)
    all_ = A.M64 if B == 64 else (1 << B) - 1
    masks = [0, all_, 1 << (B - 1), all_ ^ (1 << (B - 1))]
    masks += [int.from_bytes(rng.bytes(8), "little") & all_ for _ in range(196)]
    assert len(masks) == 200
    stu, ens, short = _decomps(B, (3, 2, 5))
    per = 5
    seen = set()
    for i, live in enumerate(masks):
        n = A.popcll(live)
        slots = B * per // 2 if i < 4 else (max(n * per - 1, 0), n * per, 2048)[i % 3]  # just past, on, far inside the threshold
        seen.add(P.check_map(all_, live, stu, ens, short, 2, slots))
        P.check_map(all_, live, stu, None, None, 2, B)
    assert seen == {False, True}


def test_threshold_both_sides_of_equality():
    """A exactly when live * (per_stu + per_ens) <= slots"""
    B = 9
    stu, ens, short = _decomps(B, (6, 6, 15))
    assert not P.short_ens(0, stu, ens, 2, 0) and not P.short_ens(0, stu, None, 2, 0)  # no live sample: nothing to arrange
    for n in range(1, B + 1):
        live = (1 << n) - 1
        total = n * 12
        assert not P.short_ens(live, stu, ens, 2, total)           # equality: one round holds both
        assert not P.short_ens(live, stu, ens, 2, total + 1)
        assert P.short_ens(live, stu, ens, 2, total - 1)
        assert not P.short_ens(live, stu, ens, 0, 0) and not P.short_ens(live, stu, ens, 1, 0)
        # --no_ens: the student's tasks alone are counted
        assert not P.short_ens(live, stu, None, 2, n * 6) and P.short_ens(live, stu, None, 2, n * 6 - 1)
        for slots in (total - 1, total, total + 1):
            assert P.check_map((1 << B) - 1, live, stu, ens, short, 2, slots) == (slots < total)


def test_the_shapes_of_the_device_tests():
    """the decompositions the device tests rely on (tests/test_gpu_pair_backfill.py), from the restated march_decompose"""
    stu, ens = A.decompose(2, 40, 130, True, device_cus=1), A.decompose(2, 40, 130, False, device_cus=1)
    short = P.decompose_short(2, 40, 130)
    assert (stu.ntasks, ens.ntasks, short.segs, short.ntasks) == (6, 6, 5, 30) and P.slots_of(1) == 8
    assert P.arrangement_of((0, 0), 2, 40, 130, device_cus=1) == "B" and P.arrangement_of((1, 0), 2, 40, 130, device_cus=1) == "A"
    # B=3 37x50: 6 + 6 tasks; two live samples sit exactly ON the threshold (8 tasks, 8 slots); ragged last short segment
    assert P.decompose_short(3, 37, 50).segs == 5 and 37 % 8 != 0
    assert [P.arrangement_of(p, 3, 37, 50, device_cus=1) for p in ((0, 0, 0), (1, 0, 0), (1, 1, 0))] == ["B", "A", "A"]
    # the headline: 165 + 165 tasks per sample, 2048 slots: A up to six live samples
    assert [P.arrangement_of((1,) * d + (0,) * (12 - d), 12, 192, 640) for d in (3, 5, 6, 7)] == ["B", "B", "A", "A"]
    assert P.decompose_short(12, 192, 640).segs == 24
