"""What the augmented-sample skip's sweep shares (tests/test_aug_skip_cases.py on the CPU, tests/test_gpu_aug_skip_sweep.py on
the device): the case table, the patterns, and the launch's index arithmetic restated in Python -- march_decompose and
march_pair_qualifies (mal_amd/csrc/mal_march.hip), march_pair_kernel's map from a workgroup number to what the workgroup
does, statement for statement, and the vector / scalar predicate of the dead-sample branch of step_epilogue_block
(mal_amd/csrc/mal_step.hip).  ``branches`` names the branches of that arithmetic a case reaches.

A pattern is the augmentation mask of a batch: 1 marks an augmented sample, whose weight 1 - mask is an exact zero -- a DEAD
sample; every other sample is LIVE."""
import collections
import functools
import itertools

import numpy as np

CW_GRAD, CW_FWD = 60, 62   # output columns of a strip: the gradient pass (two-column halo), the forward pass (one)
K_TEXEL = 4                # MAL_TEXEL_FLOATS (mal_hip.h)
K_EPI_BLOCKS = 64          # kEpiBlocks (mal_step.hip): epilogue workgroups per sample
MI355X_CUS = 256           # what hipDeviceAttributeMultiprocessorCount answers there (option "device_cus" 0)
M64 = (1 << 64) - 1

Decomp = collections.namedtuple("Decomp", "B strips segs rows ntasks per_xcd")


def decompose(B, H, W, grad, march_rows=0, march_rows_fwd=0, device_cus=MI355X_CUS):
    """march_decompose: the student's pass is a gradient pass (grad=True), the ensemble's a forward pass"""
    cw = CW_GRAD if grad else CW_FWD
    strips = (W + cw - 1) // cw
    rows = march_rows if grad else (march_rows_fwd if march_rows_fwd > 0 else march_rows)
    if rows <= 0:
        slots = device_cus * 8
        rows = 8
        while rows < H and B * strips * ((H + rows - 1) // rows) > slots:
            rows += 1
    if rows < 8:
        rows = 8
    segs = (H + rows - 1) // rows
    ntasks = B * strips * segs
    return Decomp(B, strips, segs, rows, ntasks, (ntasks + 7) // 8)


def abstract_decomp(B, per_b):
    """a decomposition with per_b tasks per sample (one strip): the map reads strips * segs, ntasks' per_xcd and B only"""
    return Decomp(B, 1, per_b, 8, B * per_b, (B * per_b + 7) // 8)


def pair_qualifies(B, H, W):
    """march_pair_qualifies under the default options ("march_lean" 1, "debug" 0)"""
    return B <= 64 and H * W * (K_TEXEL * 4) < (1 << 24)


def dead_epilogue_is_vector(H, W):
    """the dead-sample branch of step_epilogue_block takes its 16-byte path (torch's allocations are 16-byte aligned)"""
    HW = H * W
    per = (HW + K_EPI_BLOCKS - 1) // K_EPI_BLOCKS
    return ((per | HW) & 3) == 0


# ---------------------------------------------------------------- march_pair_kernel, restated
def popcll(m):
    return bin(m & M64).count("1")


@functools.lru_cache(maxsize=1 << 16)
def nth_sample(mask, k):
    """the lane whose bit of `mask` is set with k set bits below it: ctz of the ballot of `mine`"""
    ballot = 0
    for lane in range(64):
        mine = ((mask >> lane) & 1) != 0 and popcll(mask & ((1 << lane) - 1)) == k
        if mine:
            ballot |= 1 << lane
    assert ballot, "k >= popcount(mask): __builtin_ctzll(0) is undefined"
    return (ballot & -ballot).bit_length() - 1


def ballot_live(scale, scale_is_mask, B):
    """the head of every wave: lane < B loads sample_scale[lane]; -> (all, live) as 64-bit masks.  `scale` is what the
    library receives: the augmentation mask (scale_is_mask) or the weight 1 - mask formed on the host"""
    v = np.asarray(scale, dtype=np.float32)
    assert v.shape == (B,)
    live_ballot = 0
    for lane in range(64):
        sc = np.float32(1.0)
        if lane < B:
            sc = np.float32(1.0) - v[lane] if scale_is_mask else v[lane]
        if lane < B and not (sc == np.float32(0.0)):
            live_ballot |= 1 << lane
    all_ = M64 if B >= 64 else (1 << B) - 1
    return all_, live_ballot & all_


def pair_grid(stu, ens):
    """(ens_blocks, stu_blocks) of march_pair_launch; ens None: --no_ens"""
    return (ens.per_xcd * 8 if ens is not None else 0), stu.per_xcd * 8


def pair_workgroup(bid, all_, live, stu, ens, stu_first, notes=None):
    """march_pair_kernel for workgroup `bid`: ("stu" | "ens", task) for a live task, ("zero", task) for a dead task of the
    student's pass that is zero-filled (march_zero_task), None for a workgroup that returns at once.  `notes`: a set that
    receives the names of the surplus branches taken."""
    ens_blocks, stu_blocks = pair_grid(stu, ens)
    first = stu_blocks if stu_first else ens_blocks
    in_first = bid < first
    student = in_first == (stu_first != 0)
    id_ = bid if in_first else bid - first
    kp = stu if student else ens
    per_b = kp.strips * kp.segs
    n_live = popcll(live) * per_b
    per_xcd_live = (n_live + 7) >> 3
    x, j = id_ & 7, id_ >> 3
    t = x * per_xcd_live + j
    if j < per_xcd_live and t < n_live:
        k = t // per_b
        return ("stu" if student else "ens", nth_sample(live, k) * per_b + (t - k * per_b))
    if not student:
        return None
    if notes is not None:
        notes.add("surplus_j" if j >= per_xcd_live else "surplus_t")
    s = (j - per_xcd_live) * 8 + x if j >= per_xcd_live else (kp.per_xcd - per_xcd_live) * 8 + (t - n_live)
    dead = ~live & all_
    if s >= popcll(dead) * per_b:
        return None
    if notes is not None:
        notes.add("zero_j" if j >= per_xcd_live else "zero_t")
    k = s // per_b
    return ("zero", nth_sample(dead, k) * per_b + (s - k * per_b))


def check_map(all_, live, stu, ens, stu_first, notes=None):
    """every live task of each sub-pass run by exactly one workgroup, every dead task of the student's zero-filled by exactly
    one, no dead task of the ensemble's touched (a workgroup returns ONE action: it cannot do two things)"""
    B = stu.B
    ens_blocks, stu_blocks = pair_grid(stu, ens)
    done = collections.Counter(a for a in (pair_workgroup(bid, all_, live, stu, ens, stu_first, notes)
                                           for bid in range(ens_blocks + stu_blocks)) if a is not None)
    want = {}
    for name, d in (("stu", stu), ("ens", ens)):
        if d is None:
            continue
        per_b = d.strips * d.segs
        for b in range(B):
            for i in range(per_b):
                if (live >> b) & 1:
                    want[(name, b * per_b + i)] = 1
                elif name == "stu":
                    want[("zero", b * per_b + i)] = 1
    assert dict(done) == want, ("B", B, "live", hex(live), "stu_first", stu_first, "ens", ens is not None,
                                "missing", sorted(set(want) - set(done))[:8], "extra", sorted(set(done) - set(want))[:8],
                                "twice", sorted(k for k, n in done.items() if n > 1)[:8])


BRANCHES = ("surplus_j", "surplus_t", "zero_j", "zero_t", "n_live == 0", "n_live == ntasks", "n_live % 8 == 0",
            "n_live % 8 != 0", "live sample >= 32", "B == 64")


def branches(case, pattern, device_cus=MI355X_CUS):
    """the branches of the merged launch's bookkeeping the (case, pattern) reaches; none where it does not qualify"""
    B, H, W = case.B, case.H, case.W
    out = set()
    if not pair_qualifies(B, H, W):
        return out
    stu = decompose(B, H, W, True, case.rows, case.rows, device_cus)
    ens = decompose(B, H, W, False, case.rows, case.rows, device_cus)
    all_, live = ballot_live(pattern, True, B)
    for d in (stu, ens):
        n_live = popcll(live) * d.strips * d.segs
        out.add("n_live == 0" if n_live == 0 else ("n_live == ntasks" if n_live == d.ntasks else "mixed"))
        out.add("n_live % 8 == 0" if n_live % 8 == 0 else "n_live % 8 != 0")
    out.discard("mixed")
    if live >> 32:
        out.add("live sample >= 32")
    if B == 64:
        out.add("B == 64")
    ens_blocks, stu_blocks = pair_grid(stu, ens)
    for bid in range(ens_blocks + stu_blocks):
        pair_workgroup(bid, all_, live, stu, ens, 0, out)
    return out


def case_branches(case):
    """... over every pattern the sweep runs on the case"""
    out = set()
    for pattern in patterns(case.B).values():
        out |= branches(case, pattern)
    return out


# ---------------------------------------------------------------- the table
Case = collections.namedtuple("Case", "name B H W rows extra why")
# rows: "march_rows" and "march_rows_fwd" (0: the device query decides); extra: also run under "side_order" 1 and --no_ens
CASES = [
    Case("b1_16x24", 1, 16, 24, 16, True, "one task per sample; all dead: no live task, every workgroup is surplus"),
    Case("b3_16x24", 3, 16, 24, 16, False, "ntasks 3 < 8, per_xcd 1"),
    Case("b8_17x61", 8, 17, 61, 8, True, "student 2 strips, ensemble 1; one-row last segment; HW odd: scalar dead epilogue"),
    Case("b9_16x62", 9, 16, 62, 8, False, "W on the forward strip width; HW 992, per 16: vector dead epilogue"),
    Case("b12_24x122_r8", 12, 24, 122, 8, True, "the headline's batch size; 3 strips against 2; 3 segments"),
    Case("b12_24x122", 12, 24, 122, 0, False, "rows chosen by the device query"),
    Case("b33_16x24", 33, 16, 24, 16, False, "sample numbers >= 32"),
    Case("b64_16x24", 64, 16, 24, 16, False, "all = ~0; lane 63"),
    Case("b64_16x61", 64, 16, 61, 8, True, "B=64 with 4 tasks per sample"),
    Case("b65_16x24", 65, 16, 24, 16, False, "outside march_pair_qualifies: a launch per pass"),
    Case("b2_32x64", 2, 32, 64, 0, False, "the golden fixture's shape (tests/test_gpu_aug_skip.py)"),
    Case("b5_40x128", 5, 40, 128, 0, False, "3 strips x 5 segments (tests/test_gpu_aug_skip.py)"),
]
MINIMUM = {(1, 16, 24, 16), (3, 16, 24, 16), (8, 17, 61, 8), (9, 16, 62, 8), (12, 24, 122, 8), (12, 24, 122, 0), (33, 16, 24, 16),
           (64, 16, 24, 16), (64, 16, 61, 8), (65, 16, 24, 16), (2, 32, 64, 0), (5, 40, 128, 0)}


def case(name):
    return next(c for c in CASES if c.name == name)


def patterns(B):
    """name -> augmentation mask (a tuple of 0 / 1), masks that coincide listed once under their first name"""
    rng = np.random.default_rng(0xa5 + B)
    p = collections.OrderedDict()
    p["none"] = [0] * B
    p["all"] = [1] * B
    p["first"] = [1] + [0] * (B - 1)
    p["last"] = [0] * (B - 1) + [1]            # only sample B-1 dead
    p["alternating"] = [(i + 1) % 2 for i in range(B)]
    p["last_live"] = [1] * (B - 1) + [0]       # only sample B-1 live
    p["bernoulli_0"] = [int(v) for v in rng.integers(0, 2, B)]
    p["bernoulli_1"] = [int(v) for v in rng.integers(0, 2, B)]
    if B >= 33:
        p["high_live"] = [1] * 32 + [0] * (B - 32)
        p["high_dead"] = [0] * 32 + [1] * (B - 32)
    if B == 12:
        for k in range(B + 1):
            p["dead_%d" % k] = [1] * k + [0] * (B - k)
    out, seen = collections.OrderedDict(), set()
    for k, v in p.items():
        if tuple(v) not in seen:
            seen.add(tuple(v))
            out[k] = tuple(v)
    return out


def all_masks(B):
    return itertools.product((0, 1), repeat=B)
