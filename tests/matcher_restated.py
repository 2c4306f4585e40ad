"""CPU restatement of upstream's instance matcher, manydepth/matcher.py:89-173 (``HungarianMatcher.
memory_efficient_forward``), for the tests of ``mal_amd.matcher``: torch for the cost matrices, numpy for the assignment.

TEST INFRASTRUCTURE ONLY.  Differences from upstream, both deliberate: the assignment is a plain O(n^3) numpy
shortest-augmenting-path solver instead of ``scipy.optimize.linear_sum_assignment`` (scipy may be absent where the GPU tests
run), and the matched pairs are emitted in ascending index of the target instance instead of CPython's iteration order of
a set.  tests/test_matcher_host.py holds it to the reference's own outputs (tests/golden/matcher_*.npz).
"""
from __future__ import annotations

import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["a", "b", "c", "d", "e", "f"]


def ellipse_masks(params, H, W):
    """(N,4) int64 rows (cy, cx, ry, rx) -> (N,H,W) bool: dy^2 rx^2 + dx^2 ry^2 <= rx^2 ry^2 in integer arithmetic
    (the same bits on every platform)."""
    params = np.asarray(params, dtype=np.int64).reshape(-1, 4)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    out = np.zeros((len(params), H, W), dtype=bool)
    for k, (cy, cx, ry, rx) in enumerate(params):
        dy, dx = yy - cy, xx - cx
        out[k] = dy * dy * rx * rx + dx * dx * ry * ry <= rx * rx * ry * ry
    return out


def load_case(tag):
    """fixture -> dict: H, W, masks_n/m/0 (bool), class_n/m/0 (int64), C1, C2 (fp32, the reference's), pairs (K,2) =
    (row of n, row of m) in ascending target order, targets (K), margin (2)."""
    z = np.load(os.path.join(GOLDEN, "matcher_%s.npz" % tag))
    H, W = int(z["H"]), int(z["W"])
    d = {"H": H, "W": W}
    for s in ("n", "m", "0"):
        d["masks_" + s] = ellipse_masks(z["ellipses_" + s], H, W)
        d["class_" + s] = z["class_" + s].astype(np.int64)
    for k in ("C1", "C2", "pairs", "targets", "margin"):
        d[k] = z[k]
    return d


def costs_fp32(masks_a, masks_t, class_a, class_t, cost_class=1.0, cost_dice=1.0):
    """matcher.py:97-140 as written, fp32 on the CPU (batch_dice_loss :19-24 included).  The fp32 sums over H*W elements
    depend on how torch splits them over threads: one thread, as the fixtures' generator ran the reference."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _costs_fp32(masks_a, masks_t, class_a, class_t, cost_class, cost_dice)
    finally:
        torch.set_num_threads(threads)


def _costs_fp32(masks_a, masks_t, class_a, class_t, cost_class, cost_dice):
    a = torch.as_tensor(masks_a).flatten(1).float()
    t = torch.as_tensor(masks_t).flatten(1).float()
    ca, ct = torch.as_tensor(class_a), torch.as_tensor(class_t)
    n_a, n_t = a.shape[0], t.shape[0]
    cost_class_m = torch.where(ca.unsqueeze(1).repeat(1, n_t) == ct.repeat(n_a, 1), 0, 1)
    inputs = a.sigmoid()
    numerator = 2 * torch.einsum("nc,mc->nm", inputs, t)
    denominator = inputs.sum(-1)[:, None] + t.sum(-1)[None, :]
    dice = 1 - (numerator + 1) / (denominator + 1)
    return (cost_class * cost_class_m + cost_dice * dice).numpy()


def costs_fp64(masks_a, masks_t, class_a, class_t, cost_class=1.0, cost_dice=1.0):
    """The same formula evaluated in fp64 on fp32 sigmoid values: binary masks, so sigmoid is 0.5f or sigmoid(1.0f) and the
    sums are exact functions of the pixel counts."""
    flat = lambda m: np.asarray(m).reshape(np.shape(m)[0], int(np.prod(np.shape(m)[1:]))) != 0  # (an empty set keeps its H*W)
    a, t = flat(masks_a), flat(masks_t)
    hw = a.shape[1]
    s1 = float(torch.sigmoid(torch.tensor(1.0, dtype=torch.float32)))
    c11 = a.astype(np.float64) @ t.astype(np.float64).T  # integers < 2^53: exact
    cnt_a, cnt_t = a.sum(1).astype(np.float64)[:, None], t.sum(1).astype(np.float64)[None, :]
    inter = 0.5 * (cnt_t - c11) + s1 * c11
    sum_a = 0.5 * (hw - cnt_a) + s1 * cnt_a
    dice = 1.0 - (2.0 * inter + 1.0) / (sum_a + cnt_t + 1.0)
    differ = (np.asarray(class_a)[:, None] != np.asarray(class_t)[None, :]).astype(np.float64)
    return cost_class * differ + cost_dice * dice


def linear_sum_assignment(C, return_duals=False):
    """Rectangular assignment by shortest augmenting paths with duals (Crouse 2016, the algorithm scipy runs), fp64.
    Returns (row_ind, col_ind), sorted by row, min(rows, cols) pairs.  The rule mal_match.hip states and follows: the
    reduced cost ``min_val + C[i, j] - u[i] - v[j]`` is formed in fp64 in that order, and of several columns at the minimum the
    LOWEST INDEX is scanned next.  ``return_duals``: also (u, v) in the orientation of ``C`` (one per row, one per column;
    the duals of the side that is augmented over are free, those of the other side are <= 0)."""
    C = np.asarray(C, dtype=np.float64)
    if C.ndim != 2:
        raise ValueError("expected a matrix")
    if C.size == 0:
        empty = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        return empty + (np.zeros(C.shape[0]), np.zeros(C.shape[1])) if return_duals else empty
    transpose = C.shape[1] < C.shape[0]
    if transpose:
        C = C.T
    nr, nc = C.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1), np.full(nc, -1)
    for cur in range(nr):
        spc = np.full(nc, np.inf)
        path = np.full(nc, -1)
        SR, SC = np.zeros(nr, bool), np.zeros(nc, bool)
        i, sink, min_val = cur, -1, 0.0
        while sink < 0:
            SR[i] = True
            r = min_val + C[i] - u[i] - v
            better = ~SC & (r < spc)
            spc[better], path[better] = r[better], i
            j = int(np.argmin(np.where(SC, np.inf, spc)))  # the lowest index on a tie
            min_val = spc[j]
            if not np.isfinite(min_val):
                raise ValueError("cost matrix is infeasible")
            SC[j] = True
            if row4col[j] < 0:
                sink = j
            else:
                i = row4col[j]
        u[cur] += min_val
        for i in np.nonzero(SR)[0]:
            if i != cur:
                u[i] += min_val - spc[col4row[i]]
        v[SC] -= min_val - spc[SC]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    rows, cols = np.arange(nr, dtype=np.int64), col4row.astype(np.int64)
    if transpose:
        order = np.argsort(cols)
        rows, cols, u, v = cols[order], rows[order], v, u
    return (rows, cols, u, v) if return_duals else (rows, cols)


def certify(C, rows, cols, u, v, tol=1e-12):
    """The optimality certificate of an assignment (complementary slackness of the assignment LP), stated for the side the
    solver augments over as "rows": u_i + v_j <= C_ij + tol everywhere with equality (within tol) on the assigned edges,
    v <= 0, v = 0 on unassigned columns; every row assigned once, the columns distinct.  Returns the duality gap
    sum C[assigned] - (sum u + sum v) (zero up to rounding for an optimum)."""
    C = np.asarray(C, dtype=np.float64)
    rows, cols, u, v = np.asarray(rows), np.asarray(cols), np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if C.shape[1] < C.shape[0]:
        C, rows, cols, u, v = C.T, cols, rows, v, u
    nr, nc = C.shape
    assert len(rows) == nr and sorted(rows.tolist()) == list(range(nr)) and len(set(cols.tolist())) == nr
    assert C.size == 0 or float((u[:, None] + v[None, :] - C).max()) <= tol
    assert float(np.abs(u[rows] + v[cols] - C[rows, cols]).max(initial=0.0)) <= tol
    assert float(v.max(initial=0.0)) <= 0.0
    free = np.ones(nc, bool)
    free[cols] = False
    assert not v[free].any()
    return float(C[rows, cols].sum() - u.sum() - v.sum())


def margin_of(C):
    """smallest increase in the optimal total cost when one chosen edge is forbidden (fp64)"""
    C = np.asarray(C, dtype=np.float64)
    if C.size == 0:
        return np.inf
    rows, cols = linear_sum_assignment(C)
    best = C[rows, cols].sum()
    worst = np.inf
    for i, j in zip(rows, cols):
        D = C.copy()
        D[i, j] = 1e6
        r2, c2 = linear_sum_assignment(D)
        worst = min(worst, D[r2, c2].sum() - best)
    return worst


def intersect(idx_n, idx_0, idx_m, idx_1):
    """matcher.py:151-170 with the pairs in ascending target order: (pairs (K,2) int64, targets (K) int64)."""
    row_n = {int(j): int(i) for i, j in zip(idx_n, idx_0)}
    row_m = {int(j): int(i) for i, j in zip(idx_m, idx_1)}
    targets = sorted(set(row_n) & set(row_m))
    pairs = np.array([(row_n[j], row_m[j]) for j in targets], dtype=np.int64).reshape(-1, 2)
    return pairs, np.array(targets, dtype=np.int64)


def match(C1, C2):
    return intersect(*linear_sum_assignment(C1), *linear_sum_assignment(C2))


def assignment_cost(C, rows, cols):
    return float(np.asarray(C, dtype=np.float64)[np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)].sum())
