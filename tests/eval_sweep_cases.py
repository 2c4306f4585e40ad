"""The case table of the validation-metric sweep (tests/test_eval_sweep_cases.py proves each case's property on the CPU,
tests/test_gpu_eval_sweep.py holds csrc/mal_eval.hip to the oracle on them).  Seeded numpy and tests/eval_oracle.py only:
no device, no fixture.

A case is one DepthEvaluator's worth of images: ground truth (kept as float64, cast per run), raw sigmoid disparities of
one size, the split and the options.  Families: A the radix select (ground truth of the disparity's size, so the resize
is the identity and the disparity alone fixes the predictions), B the resize borders, C the dense window at its smallest,
D the options, E placement, F compute_errors.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from tests import eval_oracle as EO

ERR_SIZES = (1, 63, 64, 65, 255, 256, 257, 1025, 262143, 262144, 262145, 262401)  # 262144 = kErrBlocks * kErrThreads
ERR_TAGS = ("f64_f32", "f32_f32", "f64_f64", "f32_f64")  # gt_pred
THRESHOLDS = (1.25, 1.5625, 1.953125)                    # exact in float32 and float64
DENSE_HEIGHTS = (344, 345, 346, 350)  # round(0.75 H) = 258, 259 (258.75), 260 (259.5: both roundings agree), 262 (262.5: half to even)
DENSE_WIDTHS = (1857, 2048)
DENSE_MASKS = ("all", "one", "checker", "head")
DENSE_DISPS = ((12, 32), (24, 64))
RESIZE_SIZES = (((1, 1), (9, 13)), ((1, 7), (9, 13)), ((5, 1), (9, 13)), ((2, 2), (9, 13)), ((6, 10), (6, 10)),
                ((6, 10), (7, 11)), ((3, 5), (12, 20)), ((24, 64), (93, 310)))


def case(name, family, gts, disp, split="other", ms=True, sf=1.0, disp_max=80.0, min_depth=EO.MIN_VAL, max_depth=EO.MAX_VAL,
         which="student"):
    disp = np.ascontiguousarray(disp, np.float32)
    assert disp.ndim == 4 and disp.shape[1] == 1 and len(gts) == len(disp)
    gts = [g if g.dtype == np.float32 else np.asarray(g, np.float64) for g in gts]  # float32 (the dense images) is exact in float64
    return SimpleNamespace(name=name, family=family, gts=gts, disp=disp, split=split, ms=ms,
                           sf=sf, disp_max=disp_max, min_depth=min_depth, max_depth=max_depth, which=which)


def gts_of(c, gt_f64):
    """the case's ground truth in the run's dtype (every value used here is far enough from the mask's bounds that the cast
    to float32 keeps the mask)"""
    return [g.astype(np.float64 if gt_f64 else np.float32, copy=False) for g in c.gts]


def accumulate_kw(c):
    """the keyword arguments of DepthEvaluator.accumulate for the case (the teacher has no scale factor)"""
    return dict(disp_max=c.disp_max, median_scaling=c.ms, scale_factor=1.0 if c.which == "mono" else c.sf)


def scaled(c):
    return EO.disp_to_depth(c.disp[:, 0], 1e-3, c.disp_max)[0]


_ORACLE = {}


def oracle(c, gt_f64, cr_log=True):
    """-> (errors (N, 7) float64, ratios or None, counts, per-image oracle results), computed once per case and dtype"""
    key = (c.name, bool(gt_f64), bool(cr_log))
    if key not in _ORACLE:
        gts, sd = gts_of(c, gt_f64), scaled(c)
        res = [EO.evaluate_image(gts[i], sd[i], c.split, c.ms, None if c.which == "mono" else c.sf, min_depth=c.min_depth,
                                 max_depth=c.max_depth, cr_log=cr_log) for i in range(len(gts))]
        errs = np.array([np.array(r["errors"], np.float64) for r in res])
        ratios = np.array([r["ratio"] for r in res]) if c.ms else None
        _ORACLE[key] = (errs, ratios, np.array([r["n"] for r in res], np.int64), res)
    return _ORACLE[key]


def raw_predictions(c, i):
    """the oracle's predictions of image i before ratio and clamp (float32; what the select sees)"""
    r = EO.evaluate_image(c.gts[i], scaled(c)[i], c.split, False, None if c.which == "mono" else c.sf, min_depth=1e-30,
                          max_depth=1e30)
    assert r["n"] == oracle(c, True)[2][i], "the wide mask changed the valid set"
    return r["pred"]


def select_facts(c, i):
    """what the radix select meets in image i, from the oracle's pre-ratio predictions: n, k1 = (n - 1) // 2, the lower
    middle's bits v1, count(<= v1) (the kernel's (k1 - k) + cnt_eq), whether the min pass runs, the distinct bit patterns"""
    u = np.sort(raw_predictions(c, i).view(np.uint32))
    n = int(u.size)
    k1 = (n - 1) // 2
    v1 = int(u[k1])
    le = int((u <= v1).sum())
    return SimpleNamespace(n=n, k1=k1, v1=v1, count_le=le, min_pass=(n % 2 == 0 and le < k1 + 2), bits=u,
                           distinct=int(np.unique(u).size), bin12=v1 >> 20, mid12=(v1 >> 8) & 0xfff)


def _sparse_gt(rng, h, w, n):
    """(h, w) float64 ground truth with exactly n valid points at seeded positions, depths 2..70"""
    gt = np.zeros(h * w)
    gt[rng.permutation(h * w)[:n]] = 2.0 + 68.0 * rng.random(n)
    return gt.reshape(h, w)


def _full_gt(rng, h, w):
    return 2.0 + 60.0 * rng.random((h, w))


def _ramp(start, n):
    """n consecutive float32 values from start"""
    return (np.float32(start).view(np.uint32) + np.arange(n, dtype=np.uint32)).view(np.float32)


# ---------------------------------------------------------------- A: the select
A4_FAR = (0.002, 0.004)                       # predictions 0.497 and 0.249: different exponents
A4_LOW = tuple(_ramp(0.003, 41)[[0, 40]])     # predictions that differ in their low byte only


@functools.lru_cache(None)
def select_cases():
    out = []
    rng = np.random.default_rng(101)
    out.append(case("A1_n1to4", "A", [_sparse_gt(rng, 6, 10, n) for n in (1, 2, 3, 4)], EO.disparities(102, 4, 6, 10)))
    ramp = _ramp(0.003, 60).reshape(1, 1, 6, 10)
    full, odd = _full_gt(rng, 6, 10), _full_gt(rng, 6, 10)
    odd[3, 4] = 0.0
    out.append(case("A2_low_byte", "A", [full, odd], np.concatenate([ramp, ramp])))
    wide = np.geomspace(1e-6, 1.0, 60).astype(np.float32)[rng.permutation(60)].reshape(1, 1, 6, 10)
    out.append(case("A3_wide", "A", [full, odd], np.concatenate([wide, wide]), sf=30.0))
    gts, disps = [], []
    for (a, b), na in ((A4_FAR, 5), (A4_LOW, 5), (A4_FAR, 6), (A4_FAR, 4), (A4_LOW, 6), (A4_LOW, 4)):
        gt = _sparse_gt(rng, 6, 10, 10)
        d = np.full(60, 0.0035, np.float32)       # the other 50 pixels: never read through an identity resize
        pos = np.nonzero(gt.reshape(-1))[0][rng.permutation(10)]
        d[pos[:na]], d[pos[na:]] = a, b
        gts.append(gt)
        disps.append(d.reshape(1, 6, 10))
    out.append(case("A4_two_valued", "A", gts, np.stack(disps)))
    counts = (1023, 1024, 1025, 2049)
    out.append(case("A5_workgroup", "A", [_sparse_gt(rng, 36, 64, n) for n in counts], EO.disparities(103, 4, 36, 64)))
    return tuple(out)


A4_KINDS = ("5+5 far", "5+5 low byte", "6+4 far", "4+6 far", "6+4 low byte", "4+6 low byte")


# ---------------------------------------------------------------- B: the resize borders
@functools.lru_cache(None)
def resize_cases():
    out = []
    rng = np.random.default_rng(201)
    for k, ((sh, sw), (gh, gw)) in enumerate(RESIZE_SIZES):
        gts = [_full_gt(rng, gh, gw) for _ in range(2)]
        disp = EO.disparities(210 + k, 2, sh, sw)
        out.append(case("B_%dx%d_to_%dx%d" % (sh, sw, gh, gw), "B", gts, disp))
        if (sh, sw) == (24, 64):
            out.append(case("B_%dx%d_to_%dx%d_eigen" % (sh, sw, gh, gw), "B", gts, disp, split="eigen"))
    return tuple(out)


def resize_hits(c, i=0):
    """how many valid points of image i take each border path of resize_at: the sx < 0 branch, the right-border copy, a
    clamped first row, a clamped last row with a non-zero weight"""
    _, (gh, gw), (ys, xs), _ = EO.valid_points(c.gts[i], c.split, c.min_depth, c.max_depth)
    sh, sw = c.disp.shape[2:]
    sx, _ = EO._taps(gw, sw)
    copy = EO._columns(sw, gw)[2]
    sy, fy = EO._taps(gh, sh)
    return dict(left=int((sx[xs] < 0).sum()), copy=int(copy[xs].sum()), first_row=int((sy[ys] < 0).sum()),
                last_row=int(((sy[ys] + 1 > sh - 1) & (fy[ys] != 0)).sum()))


# ---------------------------------------------------------------- C: the dense window at its smallest
def dense_index():
    """(height, width, mask) of the images of a dense case, in order"""
    return [(h, w, m) for h in DENSE_HEIGHTS for w in DENSE_WIDTHS for m in DENSE_MASKS]


@functools.lru_cache(None)
def dense_case(dh, dw):
    rng = np.random.default_rng(301 + dh)
    y0, x0, x1 = EO.CITYSCAPES_WINDOW
    gts = []
    for h, w, m in dense_index():
        gt = (2.0 + 75.0 * rng.random((h, w))).astype(np.float32)   # valid everywhere, also outside the window
        win = gt[y0:int(round(h * 0.75)), x0:x1]                    # a view
        if m == "one":
            keep = (int(rng.integers(win.shape[0])), int(rng.integers(1024, win.shape[1])))
            v = win[keep]
            win[:] = 0.0
            win[keep] = v
        elif m == "checker":
            yy, xx = np.indices(win.shape)
            win[(yy + xx) % 2 == 1] = 0.0
        elif m == "head":
            win[0, :1024] = 0.0
        gts.append(gt)
    return case("C_dense_%dx%d" % (dh, dw), "C", gts, EO.disparities(310 + dh, len(gts), dh, dw), split="cityscapes")


def dense_cases():
    return tuple(dense_case(h, w) for h, w in DENSE_DISPS)


# ---------------------------------------------------------------- D: the options
@functools.lru_cache(None)
def option_cases():
    gts = EO.kitti_gt(401, 4, sizes=[(40, 120), (41, 121)], density=0.2)
    disp, mono = EO.disparities(402, 4, 24, 64), EO.disparities(403, 4, 24, 64)
    kw = dict(min_depth=0.1, max_depth=50)
    return (case("D_clamps", "D", gts, disp, **kw),
            case("D_teacher_100", "D", gts, mono, disp_max=100.0, which="mono", **kw),
            case("D_teacher_100_default_clamps", "D", gts, mono, disp_max=100.0, which="mono"),
            case("D_unscaled_0.5", "D", gts, disp, ms=False, sf=0.5, **kw),
            case("D_unscaled_30", "D", gts, disp, ms=False, sf=30.0, **kw))


def clamped(c, gt_f64=True):
    """-> (predictions clamped at the case's min_depth, at its max_depth) over the case's images"""
    res = oracle(c, gt_f64)[3]
    return (sum(int((r["pred"] == np.float32(c.min_depth)).sum()) for r in res),
            sum(int((r["pred"] == np.float32(c.max_depth)).sum()) for r in res))


# ---------------------------------------------------------------- E: placement
@functools.lru_cache(None)
def placement_cases():
    """seven images of A and B on 6x10 disparities (ground truth 6x10, 7x11, 9x13; 1 to 143 valid points) in one evaluator,
    as the student and as the teacher"""
    a = {c.name: c for c in select_cases()}
    rng = np.random.default_rng(501)
    gts = [a["A1_n1to4"].gts[0], a["A1_n1to4"].gts[3], a["A2_low_byte"].gts[1], a["A4_two_valued"].gts[0],
           _full_gt(rng, 6, 10), _full_gt(rng, 7, 11), _full_gt(rng, 9, 13)]
    disp = np.concatenate([a["A1_n1to4"].disp[[0, 3]], a["A2_low_byte"].disp[[1]], a["A4_two_valued"].disp[[0]],
                           EO.disparities(502, 3, 6, 10)])
    return (case("E_student", "E", gts, disp), case("E_mono", "E", gts, EO.disparities(503, 7, 6, 10), disp_max=100.0, which="mono"))


def evaluator_cases():
    return select_cases() + resize_cases() + dense_cases() + option_cases() + placement_cases()


# ---------------------------------------------------------------- F: compute_errors
def _dtypes(tag):
    g, p = tag.split("_")
    return (np.float64 if g == "f64" else np.float32), (np.float64 if p == "f64" else np.float32)


@functools.lru_cache(None)
def errors_inputs(n, tag):
    """gt 2..70, pred within a factor 2 of it (a1..a3 all strictly between 0 and 1 once n is large)"""
    rng = np.random.default_rng(600 + n % 997)
    gd, pd = _dtypes(tag)
    gt = 2.0 + 68.0 * rng.random(n)
    pred = gt * 2.0 ** rng.uniform(-1.0, 1.0, n)
    return gt.astype(gd), pred.astype(pd)


PLACEMENTS = ("below", "on", "above")


def threshold_inputs(tag, placement):
    """six points: gt / pred and pred / gt on each of 1.25, 1.5625, 1.953125 (placement "on"), or one ulp of the carrying
    array's dtype below / above it.  The other value is 1, so the quotient is the planted value exactly in every dtype."""
    gd, pd = _dtypes(tag)

    def planted(dt):
        t = np.array(THRESHOLDS, dt)
        return {"on": t, "below": np.nextafter(t, dt(0)), "above": np.nextafter(t, dt(4))}[placement]
    gt = np.concatenate([planted(gd), np.ones(3, gd)])
    pred = np.concatenate([np.ones(3, pd), planted(pd)])
    return gt, pred
