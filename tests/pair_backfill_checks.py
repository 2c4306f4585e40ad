"""What the tests of the merged launch's second arrangement share (tests/test_pair_backfill_map.py on the CPU,
tests/test_gpu_pair_backfill.py on the device): march_pair_launch's grid and march_pair_kernel's map from a workgroup number to
what the workgroup does under option "side_order" 0 / 1 / 2 (mal_amd/csrc/mal_march.hip), restated in Python statement for
statement on top of tests/aug_skip_checks.py (decompositions, the ballot, nth_sample).

Arrangement A is the map of tests/aug_skip_checks.py::pair_workgroup.  Arrangement B -- taken under "side_order" 2 when the live
tasks of both sub-passes exceed one resident round of wave slots -- puts the student's tasks first and runs the ensemble pass
behind them from its SHORT decomposition (8-row segments)."""
import collections

from tests import aug_skip_checks as A

SHORT_ROWS = 8  # kPairShortRows


def slots_of(device_cus=A.MI355X_CUS):
    """march_slots: CUs x 4 SIMDs x 2 waves"""
    return device_cus * 8


def decompose_short(B, H, W):
    """the ensemble pass in SHORT_ROWS-row segments: march_decompose with the row count given"""
    return A.decompose(B, H, W, False, SHORT_ROWS, SHORT_ROWS)


def pair_grid(stu, ens, ens_short):
    """workgroups of march_pair_launch; ens / ens_short None: --no_ens"""
    ens_blocks = ens.per_xcd * 8 if ens is not None else 0
    short_blocks = ens_short.per_xcd * 8 if ens is not None else 0
    return stu.per_xcd * 8 + max(ens_blocks, short_blocks)


def short_ens(live, stu, ens, order, slots):
    """whether the kernel takes arrangement B for the live set"""
    per_b_ens = ens.strips * ens.segs if ens is not None else 0
    return order == 2 and A.popcll(live) * (stu.strips * stu.segs + per_b_ens) > slots


def pair_workgroup(bid, all_, live, stu, ens, ens_short, order, slots):
    """march_pair_kernel for workgroup `bid`: ("stu" | "ens" | "ens_short", task) for a live task, ("zero", task) for a dead
    task of the student's pass that is zero-filled, None for a workgroup that returns at once"""
    ens_blocks_a = ens.per_xcd * 8 if ens is not None else 0
    short_blocks = ens_short.per_xcd * 8 if ens is not None else 0
    stu_blocks = stu.per_xcd * 8
    short = short_ens(live, stu, ens, order, slots)
    stu_first = short or order == 1
    ens_blocks = short_blocks if short else ens_blocks_a
    first = stu_blocks if stu_first else ens_blocks
    in_first = bid < first
    student = in_first == stu_first
    id_ = bid if in_first else bid - first
    if id_ >= (stu_blocks if student else ens_blocks):
        return None
    kp = stu if student else (ens_short if short else ens)
    per_b = kp.strips * kp.segs
    n_live = A.popcll(live) * per_b
    per_xcd_live = (n_live + 7) >> 3
    x, j = id_ & 7, id_ >> 3
    t = x * per_xcd_live + j
    if j < per_xcd_live and t < n_live:
        k = t // per_b
        name = "stu" if student else ("ens_short" if short else "ens")
        return (name, A.nth_sample(live, k) * per_b + (t - k * per_b))
    if not student:
        return None
    s = (j - per_xcd_live) * 8 + x if j >= per_xcd_live else (kp.per_xcd - per_xcd_live) * 8 + (t - n_live)
    dead = ~live & all_
    if s >= A.popcll(dead) * per_b:
        return None
    k = s // per_b
    return ("zero", A.nth_sample(dead, k) * per_b + (s - k * per_b))


def check_map(all_, live, stu, ens, ens_short, order, slots):
    """every live task of the student's pass and of the ensemble decomposition the arrangement uses run by exactly one
    workgroup, every dead task of the student's zero-filled by exactly one, nothing else touched; -> whether B was taken"""
    B = stu.B
    short = short_ens(live, stu, ens, order, slots)
    done = collections.Counter(a for a in (pair_workgroup(bid, all_, live, stu, ens, ens_short, order, slots)
                                           for bid in range(pair_grid(stu, ens, ens_short))) if a is not None)
    want = {}
    parts = [("stu", stu)]
    if ens is not None:
        parts.append(("ens_short", ens_short) if short else ("ens", ens))
    for name, d in parts:
        per_b = d.strips * d.segs
        for b in range(B):
            for i in range(per_b):
                if (live >> b) & 1:
                    want[(name, b * per_b + i)] = 1
                elif name == "stu":
                    want[("zero", b * per_b + i)] = 1
    assert dict(done) == want, ("B", B, "live", hex(live), "order", order, "slots", slots, "short", short,
                                "missing", sorted(set(want) - set(done))[:8], "extra", sorted(set(done) - set(want))[:8],
                                "twice", sorted(k for k, n in done.items() if n > 1)[:8])
    return short


def arrangement_of(pattern, B, H, W, no_ens=False, march_rows=0, march_rows_fwd=0, device_cus=A.MI355X_CUS):
    """"A" or "B": what "side_order" 2 takes for the augmentation mask `pattern` under the given options"""
    stu = A.decompose(B, H, W, True, march_rows, march_rows_fwd, device_cus)
    ens = None if no_ens else A.decompose(B, H, W, False, march_rows, march_rows_fwd, device_cus)
    _, live = A.ballot_live(pattern, True, B)
    return "B" if short_ens(live, stu, ens, 2, slots_of(device_cus)) else "A"
