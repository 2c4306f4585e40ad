"""Case tables of the segmenter sweep: mal_amd/csrc/mal_msda.hip (multi-scale deformable attention, above all its fused
route) and mal_amd/csrc/mal_instances.hip (Mask2Former's instance tail) past the shapes they were merged with.  Seeded
generators only, no fixture files; tests/test_segmenter_sweep_cases.py proves on the CPU that every case has the property
it is in its table for, tests/test_gpu_segmenter_sweep.py holds the device to the fp64 checkers (tests/msda_restated.py,
tests/instances_restated.py).

MSDA families
  M-A  both routes over (M,D) x (L,P) x ref_dim x N x Lq, offsets scaled so that about a fifth of the samples leave the map
  M-B  (device file) the fused route on a value buffer 4 bytes off the 16-byte grid
  M-C  exact fused inputs: EQUAL to the rounded fp64 checker
  M-D  softmax extremes on the fused route
  M-E  directed borders on the plain route, exact grid: EQUAL
  M-F  the segmenter's own level table at 192x640
Instances families
  I-A  multi-block grids with a ragged last block; the dword store route with a cropped H
  I-B  selection edges: topk 1, topk Q*K, filters that drop the first 64 slots or every other one
  I-C  class probabilities that round to an fp32 denormal or to zero: the rule is the ROUNDED score
  I-D  magnitudes: planes x 2^100, x 2^-100, one general fp32 plane set under the band rule"""
import functools

import numpy as np

from tests import instances_restated as IR
from tests import msda_restated as MR

# ======================================================================================================================= MSDA
MSDA_THREADS, MSDA_LDS_FLOATS = 256, 4096  # include/mal_hip.h, mal_msda_plan: a workgroup's threads and its LDS budget

MA_MD = [(8, 32), (1, 4), (3, 5), (2, 64), (2, 63)]
MA_LP = [(1, 1), (3, 4), (4, 4), (4, 8), (8, 4), (8, 1)]
MA_REF_DIMS, MA_NS, MA_LQS = (2, 4), (1, 3), (1, 63, 65, 257)
MA_BANDS = ("float4", "one_channel", "rows_by_threads", "rows_by_lds", "rows_by_total", "ragged_last_workgroup",
            "workgroup_spans_two_samples", "lanes_per_row_do_not_divide_256")


def ma_cases():
    """every (N, Lq, M, D, L, P, ref_dim) of family M-A"""
    return [(N, Lq, M, D, L, P, rd) for (M, D) in MA_MD for (L, P) in MA_LP for rd in MA_REF_DIMS for N in MA_NS for Lq in MA_LQS]


def msda_plan(N, S, Lq, M, D, L, P, aligned=True):
    from mal_amd import msda
    return msda.plan(N, S, Lq, M, D, L, P, aligned)


def msda_bands(N, Lq, M, D, L, P, S, aligned=True):
    """the bands of MA_BANDS a launch fills, from mal_msda_plan and the two limits the header states"""
    vec, rows, blocks, lds = msda_plan(N, S, Lq, M, D, L, P, aligned)
    lpr, total = D // vec, N * Lq * M
    by_threads, by_lds = MSDA_THREADS // lpr, MSDA_LDS_FLOATS // (3 * L * P + 1)
    hit = {"float4" if vec == 4 else "one_channel"}
    if rows == by_threads and by_threads < by_lds and by_threads <= total:
        hit.add("rows_by_threads")
    if rows == by_lds and by_lds < by_threads and by_lds <= total:
        hit.add("rows_by_lds")
    if rows == total and total < min(by_threads, by_lds):
        hit.add("rows_by_total")
    if total % rows and blocks > 1:
        hit.add("ragged_last_workgroup")
    first = np.arange(blocks, dtype=np.int64) * rows
    last = np.minimum(first + rows, total) - 1
    if (first // (Lq * M) != last // (Lq * M)).any():
        hit.add("workgroup_spans_two_samples")
    if MSDA_THREADS % lpr:
        hit.add("lanes_per_row_do_not_divide_256")
    return hit


def fused_inputs(seed, N, Lq, M, D, levels, P, ref_dim, spread=0.2):
    """seeded inputs of the fused route -> value, start, offsets (N,Lq,M,L,P,2), logits (N,Lq,M,L*P), reference points
    (N,Lq,L,ref_dim), fp32.  The locations they give lie around random centres with a spread that puts about a fifth
    outside [0,1], as msda_restated.sweep_inputs does for the plain route."""
    rng = np.random.default_rng(seed)
    L = len(levels)
    start, S = MR.starts_of(levels)
    value = rng.standard_normal((N, S, M, D)).astype(np.float32)
    ref = rng.random((N, Lq, 1, 2)) + 0.02 * rng.standard_normal((N, Lq, L, 2))
    u = spread * rng.standard_normal((N, Lq, M, L, P, 2))
    if ref_dim == 2:   # location = ref + off / (W, H)
        off = u * np.array([[w, h] for h, w in levels], np.float64)[None, None, None, :, None, :]
    else:              # location = ref[:2] + off / P * ref[2:] * 0.5
        box = rng.uniform(0.2, 0.6, (N, Lq, L, 2))
        off = u * P / (0.5 * box[:, :, None, :, None, :])
        ref = np.concatenate([ref, box], -1)
    logits = rng.standard_normal((N, Lq, M, L * P))
    return value, start, off.astype(np.float32), logits.astype(np.float32), ref.astype(np.float32)


def fused_chain(value, levels, start, off, logits, ref, dtype):
    """the fused route's function in ``dtype``: softmax, location step, operator -> (output, locations, weights)"""
    N, Lq, M, L, P = off.shape[:5]
    with np.errstate(invalid="ignore", over="ignore"):
        loc = MR.locations(off, ref, levels, dtype)
        w = MR.softmax(logits, dtype).reshape(N, Lq, M, L, P)
    return MR.core(value, levels, start, loc, w, dtype), loc, w


def inside_fraction(loc, levels):
    """share of the samples that pass the range test, fp64"""
    loc = np.asarray(loc, np.float64)
    hit = total = 0
    for l, (H, W) in enumerate(levels):
        x, y = loc[:, :, :, l, :, 0] * W - 0.5, loc[:, :, :, l, :, 1] * H - 0.5
        hit += int(((y > -1) & (x > -1) & (y < H) & (x < W)).sum())
        total += x.size
    return hit / total


def ma_inputs(N, Lq, M, D, L, P, ref_dim):
    levels = MR.SWEEP_LEVELS[L]
    seed = 100003 * ref_dim + 10007 * N + 101 * Lq + 31 * M + D + 1009 * L + 13 * P
    return (levels,) + fused_inputs(seed, N, Lq, M, D, levels, P, ref_dim)


# ---- M-C: exact fused inputs.  Level sizes are powers of two >= 4: a location has resolution 2^-8 at worst (offset 2^-2,
# / P <= 8, x box >= 2^-2, x 0.5), so x W - 0.5 has 2^-6, a corner weight 2^-12, times an integer value |v| <= 64 and the
# weight 1/LP >= 2^-5: every term and every partial sum is a multiple of 2^-17 below 2^6 in magnitude, 23 bits
MC_LEVELS = {1: ((8, 16),), 2: ((8, 16), (4, 8)), 4: ((8, 16), (4, 8), (4, 4), (16, 4)),
             8: ((8, 16), (4, 8), (4, 4), (16, 4), (8, 8), (4, 16), (32, 4), (4, 32))}
#            ref_dim, L, P: every L*P in {1, 2, 4, 8, 16, 32}
MC_CASES = [(4, 4, 8), (4, 8, 4), (4, 2, 1), (4, 4, 4), (2, 1, 1), (2, 2, 1), (2, 2, 2), (2, 2, 4), (2, 4, 4), (2, 8, 4)]
MC_MD = [(3, 8), (2, 5)]  # float4 and one channel; 37 queries x 3 heads: workgroups that span both samples


def mc_inputs(ref_dim, L, P, M, D, N=2, Lq=37):
    rng = np.random.default_rng(5000 + 100 * ref_dim + 10 * L + P + M)
    levels = MC_LEVELS[L]
    start, S = MR.starts_of(levels)
    value = rng.integers(-64, 65, (N, S, M, D)).astype(np.float32)
    ref = rng.integers(-2, 35, (N, Lq, L, 2)) / 32.0
    if ref_dim == 2:
        off = rng.integers(-12, 13, (N, Lq, M, L, P, 2)) / 4.0
    else:
        off = rng.integers(-4 * P, 4 * P + 1, (N, Lq, M, L, P, 2)) / 4.0
        ref = np.concatenate([ref, 2.0 ** rng.integers(-2, 2, (N, Lq, L, 2))], -1)
    logits = np.broadcast_to(rng.integers(-3, 4, (N, Lq, M, 1)), (N, Lq, M, L * P))  # constant along a row: weights 1/LP
    return levels, value, start, off.astype(np.float32), np.ascontiguousarray(logits).astype(np.float32), ref.astype(np.float32)


# ---- M-D: softmax extremes.  (A row of all -inf is NaN in torch's softmax as well: out of scope.)
MD_SHAPES = [(2, 65, 8, 32, 4, 4, 2), (2, 65, 3, 5, 8, 4, 4)]  # N, Lq, M, D, L, P, ref_dim
MD_KINDS = ("sigma30", "sigma120", "one_minus_inf", "all_1e4", "offset_1e6")


def md_inputs(shape, kind):
    N, Lq, M, D, L, P, ref_dim = shape
    levels = MR.SWEEP_LEVELS[L]
    value, start, off, logits, ref = fused_inputs(7000 + M + MD_KINDS.index(kind), N, Lq, M, D, levels, P, ref_dim)
    rng = np.random.default_rng(7100 + M + MD_KINDS.index(kind))
    if kind == "sigma30":
        logits = (30.0 * rng.standard_normal(logits.shape)).astype(np.float32)
    elif kind == "sigma120":
        logits = (120.0 * rng.standard_normal(logits.shape)).astype(np.float32)
    elif kind == "one_minus_inf":
        at = rng.integers(0, L * P, logits.shape[:3])
        at[0, 0, 0], at[0, 1, 0] = 0, L * P - 1  # the first logit (the running maximum starts there) and the last
        np.put_along_axis(logits, at[..., None], -np.inf, -1)
    elif kind == "all_1e4":
        logits = np.full(logits.shape, 1e4, np.float32)
    elif kind == "offset_1e6":
        logits = (logits + np.float32(1e6)).astype(np.float32)  # fp32 spacing at 1e6 is 1/16: the rows stay non-constant
    return levels, value, start, off, logits, ref


# ---- M-E: directed borders on the plain route.  Locations k/128, weights k/64, integer values |v| <= 8: x W - 0.5 has
# resolution 2^-7, a corner weight 2^-14, the attention weight 2^-6, a value 3 bits: 23 bits, exact in any order
ME_LEVELS = ((1, 7), (7, 1), (1, 1), (8, 16))
ME_GRID = 128
ME_MD = [(2, 8), (1, 5)]


def me_axis(n):
    """locations (multiples of 1/128) along an axis of n texels whose pixel coordinate t = loc n - 0.5 brackets each of
    -1, -0.5, 0, an interior integer, n-1, n-0.5 and n: the grid value at or just below and at or just above each (the
    value itself where the grid holds it, which it does for every one when n is a power of two), the next grid value
    above -1 and the first at or beyond n"""
    ks = set()
    for t in (-1.0, -0.5, 0.0, float(n // 2), n - 1.0, n - 0.5, float(n)):
        k = (t + 0.5) * ME_GRID / n
        ks.update((int(np.floor(k)), int(np.ceil(k))))
    ks.add(int(np.floor(-0.5 * ME_GRID / n)) + 1)   # the next value above -1
    ks.add(int(np.ceil((n + 0.5) * ME_GRID / n)))   # the first value at or beyond n
    return np.array(sorted(ks), np.float64) / ME_GRID


def me_inputs(M, D, N=1):
    """one sample per level and query (P = 1); query q takes the q-th pair of the product (x candidates) x (y candidates) of
    its level, wrapping around: every pair of every level occurs"""
    rng = np.random.default_rng(8000 + D)
    levels = ME_LEVELS
    start, S = MR.starts_of(levels)
    axes = [(me_axis(W), me_axis(H)) for H, W in levels]
    Lq = max(len(x) * len(y) for x, y in axes)
    loc = np.empty((N, Lq, M, len(levels), 1, 2), np.float32)
    q = np.arange(Lq)
    for l, (xs, ys) in enumerate(axes):
        loc[:, :, :, l, 0, 0] = xs[q % len(xs)][None, :, None]
        loc[:, :, :, l, 0, 1] = ys[(q // len(xs)) % len(ys)][None, :, None]
    value = rng.integers(-8, 9, (N, S, M, D)).astype(np.float32)
    weights = (rng.integers(1, 17, (N, Lq, M, len(levels), 1)) / 64.0).astype(np.float32)
    return levels, value, start, loc, weights


def me_census(loc, levels):
    """per level: how often each failing side of the range test and each corner pattern (y0, y1, x0, x1) of a sample inside
    occurs, in fp64 on the exact inputs -> list of (sides dict, patterns dict, set of pixel coordinates x, of y)"""
    out = []
    for l, (H, W) in enumerate(levels):
        x = np.asarray(loc[:, :, :, l, :, 0], np.float64).ravel() * W - 0.5
        y = np.asarray(loc[:, :, :, l, :, 1], np.float64).ravel() * H - 0.5
        sides = {"y<=-1": int((y <= -1).sum()), "x<=-1": int((x <= -1).sum()), "y>=H": int((y >= H).sum()), "x>=W": int((x >= W).sum())}
        ok = (y > -1) & (x > -1) & (y < H) & (x < W)
        yl, xl = np.floor(y[ok]), np.floor(x[ok])
        pat = {}
        for p in zip(yl >= 0, yl + 1 <= H - 1, xl >= 0, xl + 1 <= W - 1):
            pat[tuple(bool(b) for b in p)] = pat.get(tuple(bool(b) for b in p), 0) + 1
        out.append((sides, pat, set(x.tolist()), set(y.tolist())))
    return out


def reachable_patterns(H, W):
    """(y0, y1, x0, x1) of a sample inside the map: the lower corner row is -1, interior or the last one"""
    ys = [(False, True), (True, False)] + ([(True, True)] if H >= 2 else [])
    xs = [(False, True), (True, False)] + ([(True, True)] if W >= 2 else [])
    return {y + x for y in ys for x in xs}


# ---- M-F: the segmenter's own table at 192x640 (strides 8, 16, 32), self-attention
MF_LEVELS, MF_M, MF_D, MF_P, MF_N = ((24, 80), (12, 40), (6, 20)), 8, 32, 4, 2


@functools.lru_cache(maxsize=None)
def mf_inputs():
    S = MR.starts_of(MF_LEVELS)[1]
    return (MF_LEVELS,) + fused_inputs(9000, MF_N, S, MF_M, MF_D, MF_LEVELS, MF_P, 2)


# ================================================================================================================== instances
INST_THREADS = 256                     # texels per workgroup of the mask launch
THING8 = np.array([1, 1, 0, 1, 1, 1, 0, 1], dtype=bool)
SMALL_PLANE = (2, 3, 7, 11)            # h, w, H, W of the families that are about the selection (byte route, one block)


def align256(n):
    return (n + 255) // 256 * 256


def inst_blocks(h, w):
    return -(-h * w // INST_THREADS)


def inst_route(w, W):
    """the store route of the mask launch for a 4-byte aligned mask buffer"""
    return "dword" if W == 4 * w else "byte"


def inst_workspace(N, Q, T, h, w):
    """mal_instances_workspace_bytes as mal_amd/csrc/mal_instances.hip lays it out: statistics, one fp64 and one int32
    partial per (image, slot, workgroup), each piece rounded up to 256 bytes, and 256 for the base's alignment"""
    parts = N * T * inst_blocks(h, w)
    return align256(N * Q * 2 * 8) + align256(parts * 8) + align256(parts * 4) + 256


def dyadic_planes(rng, N, Q, h, w):
    return rng.integers(-16 * IR.MASK_UNIT, 16 * IR.MASK_UNIT + 1, (N, Q, h, w)).astype(np.float32) / IR.MASK_UNIT


def margin_logits(rng, Q, K, T, cut=1e-5, sel=1e-6):
    """N(0, 4) class logits whose selection is no matter of rounding: the relative gap at the cut >= ``cut`` and between any
    two selected scores >= ``sel`` (fp32 rounds at 6e-8)"""
    for _ in range(400):
        logits = (rng.standard_normal((Q, K + 1)) * 2.0).astype(np.float32)
        s = np.sort(IR.class_scores(logits))[::-1]
        gaps = (s[:T - 1] - s[1:T]) / s[:T - 1]
        if (T == len(s) or (s[T - 1] - s[T]) / s[T - 1] >= cut) and (T == 1 or gaps.min() >= sel):
            return logits
    raise AssertionError("no class logits with a margin")


def ranked_logits(Q, K, order):
    """class logits whose candidates come out in the given order of flat indices q*K + c: rank r gets 10 - r/20 and the
    "no object" column 20, so that every row's sum is e^20 to 4e-4 and the 5 % steps between ranks decide; candidates
    outside ``order`` get -30"""
    logits = np.full((Q, K + 1), -30.0, np.float64)
    logits[:, K] = 20.0
    for r, e in enumerate(order):
        logits[e // K, e % K] = 10.0 - r / 20.0
    return logits.astype(np.float32)


# ---- I-A: h, w, H, W, ragged multi-block grid claimed, route claimed, cropped rows (4h - H)
IA_SHAPES = [(17, 16, 68, 64, True, "dword", 0), (17, 16, 65, 64, True, "dword", 3), (16, 17, 64, 65, True, "byte", 0),
             (33, 8, 129, 32, True, "dword", 3), (1, 257, 4, 1028, True, "dword", 0), (257, 1, 1025, 4, True, "dword", 3),
             (3, 4, 9, 16, False, "dword", 3), (3, 4, 10, 16, False, "dword", 2), (3, 4, 11, 16, False, "dword", 1)]
IA_Q, IA_K, IA_T = 5, 8, 6


@functools.lru_cache(maxsize=None)
def ia_inputs(shape, N):
    """-> logits (N,Q,K+1), planes (N,Q,h,w), thing (None at N = 1; at N = 3 a filter that leaves a different count in
    every image)"""
    h, w, H, W = shape[:4]
    rng = np.random.default_rng(11000 + 97 * h + w + 1000 * N + H)
    planes = dyadic_planes(rng, N, IA_Q, h, w)
    thing = THING8 if N == 3 else None
    for _ in range(200):
        logits = np.stack([margin_logits(rng, IA_Q, IA_K, IA_T) for _ in range(N)])
        if thing is None:
            return logits, planes, thing
        counts = [int(thing[IR.select(IR.class_scores(logits[n]), IA_T) % IA_K].sum()) for n in range(N)]
        if len(set(counts)) == N and min(counts) >= 1:
            return logits, planes, thing
    raise AssertionError("no class logits with distinct counts")


# ---- I-B: name -> (Q, K, T).  N = 2 images per case
IB_CASES = {"topk_1": (5, 8, 1), "all_1x1": (1, 1, 1), "all_3x5": (3, 5, 15), "all_16x8": (16, 8, 128)}
IB_FILTER_T = (64, 65, 128)
IB_FILTER_QK = (32, 8)


@functools.lru_cache(maxsize=None)
def ib_inputs(name):
    """-> Q, K, T, logits (2,Q,K+1), planes (2,Q,h,w), thing"""
    h, w = SMALL_PLANE[:2]
    kind, _, t = name.partition("@")
    rng = np.random.default_rng(12000 + sum(map(ord, name)))
    if kind in IB_CASES:
        Q, K, T = IB_CASES[kind]
        logits, thing = np.stack([margin_logits(rng, Q, K, T) for _ in range(2)]), None
    else:
        (Q, K), T = IB_FILTER_QK, int(t)
        per_image = []
        for n in range(2):
            if kind == "drop_first_64":   # ranks 0..63 are the 64 candidates of the classes 0 and 1, which the filter drops
                head = [q * K + c for q in range(Q) for c in (0, 1)]
                tail = [q * K + c for q in range(Q) for c in range(2, K)]
                order = list(rng.permutation(head)) + list(rng.permutation(tail))
                thing = np.arange(K) >= 2
            else:                         # "alternate": an odd multiplier keeps the parity, class parity = rank parity
                assert kind == "alternate"
                order = [(r * (37, 93)[n]) % (Q * K) for r in range(Q * K)]
                thing = np.arange(K) % 2 == 0
            per_image.append(ranked_logits(Q, K, order))
        logits = np.stack(per_image)
    return Q, K, T, logits, dyadic_planes(rng, 2, Q, h, w), thing


def ib_names():
    return list(IB_CASES) + ["%s@%d" % (k, t) for k in ("drop_first_64", "alternate") for t in IB_FILTER_T]


# ---- I-C: probabilities below fp32's normal range.  Image 0: a gap of about 95 to the row maximum (exp(-95) = 5.5e-42, an
# fp32 denormal with 12 bits: steps of 2^-14 in the logit give runs of equal fp32 values with distinct fp64 ones); image 1:
# about 120 (7.7e-53 rounds to zero).  The logits RISE with the flat index, so the fp64 order prefers the higher index and
# the rounded rule (ties to the lower index) the lower one.
IC_Q, IC_K, IC_T, IC_GAPS = 4, 6, 10, (95.0, 120.0)


@functools.lru_cache(maxsize=None)
def ic_inputs():
    rng = np.random.default_rng(13000)
    logits = np.zeros((2, IC_Q, IC_K + 1), np.float32)
    for n, gap in enumerate(IC_GAPS):
        e = np.arange(IC_Q * IC_K, dtype=np.float64).reshape(IC_Q, IC_K)
        logits[n, :, :IC_K] = (-gap + e * 2.0 ** -14).astype(np.float32)
        logits[n, 0, 1], logits[n, 2, 3] = 2.0, 1.0  # two ordinary scores in front
    return logits, dyadic_planes(rng, 2, IC_Q, *SMALL_PLANE[:2])


# ---- I-D
ID_SHAPE, ID_Q, ID_K, ID_T = (17, 16, 65, 64), 5, 8, 6
ID_GENERAL_Q, ID_GENERAL_K, ID_GENERAL_T, ID_GENERAL_SEED = 12, 2, 12, 14000


@functools.lru_cache(maxsize=None)
def id_scaled_inputs(exponent):
    """dyadic planes times 2^exponent (exact: the products stay far inside fp32's normal range)"""
    rng = np.random.default_rng(14100)
    planes = dyadic_planes(rng, 1, ID_Q, *ID_SHAPE[:2]) * np.float32(2.0 ** exponent)
    return margin_logits(rng, ID_Q, ID_K, ID_T)[None], planes


@functools.lru_cache(maxsize=None)
def id_general_inputs(seed=ID_GENERAL_SEED):
    rng = np.random.default_rng(seed)
    planes = (rng.standard_normal((1, ID_GENERAL_Q) + ID_SHAPE[:2]) * 2.0).astype(np.float32)
    return margin_logits(rng, ID_GENERAL_Q, ID_GENERAL_K, ID_GENERAL_T)[None], planes
