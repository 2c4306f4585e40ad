"""Golden vectors for the instance matcher (mal_amd/matcher.py) from the REFERENCE's own ``HungarianMatcher.forward``.

TEST INFRASTRUCTURE ONLY.  Run in the authoring container only (needs the reference checkout and scipy):

    python scripts/gen_golden_matcher.py /path/to/reference

``manydepth/matcher.py`` imports ``detectron2.structures.instances`` for a type name it never uses; the module is imported
with an inert stand-in for it (the method of oracle/gen_golden_dr.py).  The module's ``linear_sum_assignment`` name is
wrapped to record the two cost matrices and the two assignments as the reference made them; ``forward`` runs on the CPU.

Inputs are integer-arithmetic ellipses (tests/matcher_restated.ellipse_masks), so a fixture stores only their parameters,
the classes and the expected outputs: tests/golden/matcher_<case>.npz, a few KB each, data only.  The target ellipses
reappear in ``n`` and ``m`` jittered by <= 2 px, mixed with distractors and permuted.

A fixture is written only if the optimum of each matrix is UNIQUE with a margin >= 1e-4: every chosen edge is forbidden
in turn, the problem re-solved in fp64, and the smallest increase in total cost is the margin (stored).  Exact equality of
a correct solver's pairs with the reference's is then a fair demand.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import matcher_restated as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MARGIN = 1e-4
#        tag  H    W    N_n N_m N_0 classes differ
CASES = [("a", 5, 13, 3, 3, 2, False),
         ("b", 24, 40, 5, 4, 3, True),
         ("c", 32, 64, 70, 66, 6, False),
         ("d", 32, 64, 6, 6, 70, False),
         ("e", 192, 640, 20, 20, 8, False),
         ("f", 24, 40, 4, 0, 3, False)]


def import_matcher(ref):
    sys.path.insert(0, ref)
    for name in ("detectron2", "detectron2.structures", "detectron2.structures.instances"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            m.Instances = object
            sys.modules[name] = m
    import manydepth.matcher as M
    return M


class Instances:
    def __init__(self, classes, masks):
        self.pred_classes, self.pred_masks = torch.as_tensor(classes), torch.as_tensor(masks).float()

    def __len__(self):
        return len(self.pred_classes)


def random_ellipse(rng, H, W):
    ry, rx = int(rng.integers(1, max(H // 4, 2) + 1)), int(rng.integers(1, max(W // 6, 2) + 1))
    return [int(rng.integers(0, H)), int(rng.integers(0, W)), ry, rx]


def make_inputs(rng, H, W, n_n, n_m, n_0, classes_differ):
    tgt = np.array([random_ellipse(rng, H, W) for _ in range(n_0)], dtype=np.int64).reshape(-1, 4)
    cls_0 = rng.integers(0, 5, n_0)
    sides = []
    for n in (n_n, n_m):
        keep = rng.permutation(n_0)[:min(n, n_0)]  # the targets that reappear on this side
        ell = tgt[keep].copy()
        ell[:, :2] += rng.integers(-2, 3, (len(keep), 2))
        cls = cls_0[keep].copy()
        if classes_differ and len(cls):  # the class term decides for some
            flip = rng.random(len(cls)) < 0.4
            cls[flip] = (cls[flip] + 1) % 5
        extra = n - len(keep)
        if extra:
            ell = np.concatenate([ell, np.array([random_ellipse(rng, H, W) for _ in range(extra)], dtype=np.int64)])
            cls = np.concatenate([cls, rng.integers(0, 5, extra)])
        order = rng.permutation(n)
        sides.append((ell[order].reshape(-1, 4), cls[order].astype(np.int64)))
    return sides[0], sides[1], (tgt, cls_0.astype(np.int64))


margin_of = R.margin_of


def run_reference(M, n, m, t, H, W):
    from scipy.optimize import linear_sum_assignment as lsa
    rec = []

    def recording(C):
        C = np.asarray(C)
        rows, cols = lsa(C) if C.size else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        rec.append((C.copy(), np.asarray(rows), np.asarray(cols)))
        return rows, cols

    M.linear_sum_assignment = recording
    inst = [Instances(c, R.ellipse_masks(e, H, W)) for e, c in (n, m, t)]
    slice_n, slice_m = M.HungarianMatcher().forward(*inst)
    (C1, idx_n, idx_0), (C2, idx_m, idx_1) = rec
    pairs, targets = R.intersect(idx_n, idx_0, idx_m, idx_1)
    # the pairs the reference returned are these, in its own (set iteration) order
    theirs = sorted(zip(slice_n.tolist(), slice_m.tolist()))
    assert theirs == sorted(map(tuple, pairs.tolist())), (theirs, pairs)
    return C1.astype(np.float32), C2.astype(np.float32), pairs, targets


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    M = import_matcher(sys.argv[1])
    torch.set_num_threads(1)  # one summation order of the reference's fp32 sums, whatever the host
    for tag, H, W, n_n, n_m, n_0, differ in CASES:
        for seed in range(1000):
            rng = np.random.default_rng(1000 * ord(tag) + seed)
            n, m, t = make_inputs(rng, H, W, n_n, n_m, n_0, differ)
            masks = [R.ellipse_masks(e, H, W) for e, _ in (n, m, t)]
            if any(len(k) and k.reshape(len(k), -1).sum(1).min() == 0 for k in masks):
                continue  # an ellipse that misses the image
            D1 = R.costs_fp64(masks[0], masks[2], n[1], t[1])
            D2 = R.costs_fp64(masks[1], masks[2], m[1], t[1])
            margins = (margin_of(D1), margin_of(D2))
            if min(margins) >= MARGIN:
                break
        else:
            raise SystemExit("case %s: no inputs with a unique optimum (margin >= %g) found" % (tag, MARGIN))
        C1, C2, pairs, targets = run_reference(M, n, m, t, H, W)
        assert C1.dtype == np.float32 and C1.shape == (n_n, n_0) and C2.shape == (n_m, n_0)
        # the reference's fp32 matrices against the fp64 evaluation, and the reference's pairs against the fp64 optimum
        err = max([float(np.abs(C - D).max()) for C, D in ((C1, D1), (C2, D2)) if C.size] or [0.0])
        mine, _ = R.match(D1, D2)
        assert np.array_equal(mine, pairs), (tag, mine, pairs)
        np.savez(os.path.join(OUT, "matcher_%s.npz" % tag), H=np.int64(H), W=np.int64(W), ellipses_n=n[0], ellipses_m=m[0],
                 ellipses_0=t[0], class_n=n[1], class_m=m[1], class_0=t[1], C1=C1, C2=C2, pairs=pairs, targets=targets,
                 margin=np.array(margins, dtype=np.float64))
        print("case %s seed %d: %dx%d N=(%d,%d,%d) pairs %d margin %.3g / %.3g, |fp32 - fp64| <= %.3g"
              % (tag, seed, H, W, n_n, n_m, n_0, len(pairs), margins[0], margins[1], err))


if __name__ == "__main__":
    main()
