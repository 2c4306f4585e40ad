"""GPU: the validation-metric kernels (csrc/mal_eval.hip, mal_amd/evaluate.py) swept past their fixtures, on the case table
of tests/eval_sweep_cases.py (tests/test_eval_sweep_cases.py proves each case's property on the CPU): the radix select at
1..4 points, in its third pass alone, on both sides of its even-count rule and around the workgroup's 1024 threads; the
resize's border paths; the dense window at its smallest; the clamps and the teacher's range; placement; compute_errors
across its grid stride and on its thresholds.

Gates (the project's own): per-image median ratios bit-equal with their dtype; a1..a3 equal as counts and as values;
abs_rel, sq_rel, rmse, rmse_log within 1e-9 relative (float64 ground truth) / 1e-5 (float32) of the oracle with the
correctly rounded float32 log the device computes (the distance from numpy's own log is printed); an oracle 0 is a device
0; mal_eval_mean bit-equal to the in-order float64 sum of the returned rows over N."""
import numpy as np
import pytest
import torch

from tests import eval_oracle as EO
from tests import eval_sweep_cases as SC
from tests.test_gpu_eval import DEV, run_gpu, tol

pytestmark = pytest.mark.gpu
NAMES = ("abs_rel", "sq_rel", "rmse", "rmse_log")
WORST = {}   # (metric, "f64" / "f32") -> (largest relative distance from the oracle, case)


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


@pytest.fixture(scope="module", autouse=True)
def _largest_distances():
    """after the file's last test: the figures of DESIGN.md 11 "Sweep" (shown with -s)"""
    yield
    for key in sorted(WORST):
        print("largest %s %s: %.2e (%s)" % (key[0], key[1], WORST[key][0], WORST[key][1]))


def _rel(got, want):
    w = np.abs(want)
    return np.abs(got - want) / np.where(w > 0, w, 1.0)


def _note(rel, gt_f64, what):
    for k, name in enumerate(NAMES):
        key = (name, "f64" if gt_f64 else "f32")
        if key not in WORST or rel[k] > WORST[key][0]:
            WORST[key] = (float(rel[k]), what)


def mean_in_order(rows):
    """np.array(errors).mean(0) as mal_eval_mean takes it: a float64 sum in image order, one division"""
    out = []
    for k in range(7):
        s = 0.0
        for i in range(len(rows)):
            s += float(rows[i, k])
        out.append(s / float(len(rows)))
    return np.array(out, np.float64)


def hold(gpu, c, gt_f64, what=""):
    """the device's (mean, per-image errors, ratios) of case c against the oracle"""
    what = "%s %s %s" % (c.name, "f64" if gt_f64 else "f32", what)
    mean, errs, ratios = gpu
    want, want_ratios, counts, _ = SC.oracle(c, gt_f64)
    assert errs.shape == want.shape and errs.dtype == np.float64, what
    if want_ratios is None:
        assert ratios is None, what
    else:
        assert ratios.dtype == want_ratios.dtype == (np.float64 if gt_f64 else np.float32), what
        bad = np.nonzero(ratios != want_ratios)[0]
        assert bad.size == 0, "%s: ratios differ at images %s: %r vs %r" % (what, bad[:5], ratios[bad[:5]], want_ratios[bad[:5]])
    got_c = np.rint(errs[:, 4:] * counts[:, None]).astype(np.int64)
    want_c = np.rint(want[:, 4:] * counts[:, None]).astype(np.int64)
    assert (got_c == want_c).all(), "%s: a1..a3 counts differ at images %s" % (what, np.nonzero((got_c != want_c).any(1))[0][:5])
    assert (errs[:, 4:] == want[:, 4:]).all(), what
    rel = _rel(errs[:, :4], want[:, :4])
    numpy_own = SC.oracle(c, gt_f64, cr_log=False)[0]
    print("%s: max rel per metric %s; rmse_log against numpy's own log %.2e"
          % (what, ["%.1e" % v for v in rel.max(0)], _rel(errs[:, 3], numpy_own[:, 3]).max()))
    _note(rel.max(0), gt_f64, what)
    zero = want[:, :4] == 0
    assert (errs[:, :4][zero] == 0).all(), "%s: an oracle 0 is not 0 at %s" % (what, np.argwhere(zero & (errs[:, :4] != 0))[:5])
    assert (rel <= tol(gt_f64)).all(), "%s: max rel per metric %s at images %s" % (what, rel.max(0), rel.argmax(0))
    assert mean.dtype == np.float64 and mean.tobytes() == mean_in_order(errs).tobytes(), (what, mean, mean_in_order(errs))
    return rel.max(0)


def evaluator(c, gt_f64):
    from mal_amd.evaluate import DepthEvaluator
    return DepthEvaluator(SC.gts_of(c, gt_f64), c.split, DEV, min_depth=c.min_depth, max_depth=c.max_depth)


CASES = {c.name: c for c in SC.select_cases() + SC.resize_cases() + SC.dense_cases() + SC.option_cases()}


# ---------------------------------------------------------------- A to D: one evaluator per case and dtype
@pytest.mark.parametrize("gt_f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_case_matches_the_oracle(name, gt_f64):
    c = CASES[name]
    ev = evaluator(c, gt_f64)
    hold(run_gpu(ev, c.disp, c.which, **SC.accumulate_kw(c)), c, gt_f64)
    if c.family == "A":   # one image per call as well: a workgroup alone in its grid
        ev.reset()
        hold(run_gpu(ev, c.disp, c.which, batch=1, **SC.accumulate_kw(c)), c, gt_f64, "one per call")


# ---------------------------------------------------------------- E: placement
@pytest.mark.parametrize("gt_f64", [True, False], ids=["f64", "f32"])
def test_placement_orders_and_interleaving_give_the_same_bytes(gt_f64):
    cs = {c.which: c for c in SC.placement_cases()}
    ev = evaluator(cs["student"], gt_f64)
    d = {w: torch.from_numpy(c.disp).to(DEV) for w, c in cs.items()}
    plans = {"one per call, reversed": [(w, i, i + 1) for i in range(6, -1, -1) for w in ("student", "mono")],
             "3 + 4": [("student", 0, 3), ("mono", 0, 3), ("mono", 3, 7), ("student", 3, 7)],
             "4 then 3, mono first": [("mono", 3, 7), ("student", 3, 7), ("student", 0, 3), ("mono", 0, 3)],
             "one call": [("student", 0, 7), ("mono", 0, 7)]}
    first = None
    for what, plan in plans.items():
        ev.reset()
        for w, a, b in plan:
            ev.accumulate(d[w][a:b], a, w, **SC.accumulate_kw(cs[w]))
        got = {w: ev.result(w) for w in ("student", "mono")}
        for w in got:
            hold(got[w], cs[w], gt_f64, what)
        if first is None:
            first = got
        for w in got:
            for x, y in zip(got[w], first[w]):
                assert x.tobytes() == y.tobytes(), (what, w)


# ---------------------------------------------------------------- F: compute_errors
def errors_on_device(g, p):
    from mal_amd.evaluate import compute_errors
    return compute_errors(torch.from_numpy(g).to(DEV), torch.from_numpy(p).to(DEV))


def hold_errors(r, g, p, tag, what):
    want = EO.compute_errors(g, p, cr_log=True)
    assert [str(v.dtype).replace("torch.", "") for v in r] == [str(np.asarray(v).dtype) for v in want], (tag, what)
    assert all(v.dim() == 0 and v.is_cuda for v in r)
    got, want = np.array([float(v) for v in r]), np.array([float(v) for v in want])
    n = g.size
    assert (np.rint(got[4:] * n) == np.rint(want[4:] * n)).all() and (got[4:] == want[4:]).all(), (tag, what, got, want)
    rel = _rel(got[:4], want[:4])
    own = np.array([float(v) for v in EO.compute_errors(g, p)])
    print("errors %s %s: rel %s; rmse_log against numpy's own log %.2e" % (tag, what, ["%.1e" % v for v in rel], _rel(got[3], own[3])))
    _note(rel, tag != "f32_f32", "errors %s %s" % (tag, what))
    assert (got[:4][want[:4] == 0] == 0).all(), (tag, what, got, want)
    assert (rel <= (1e-5 if tag == "f32_f32" else 1e-9)).all(), (tag, what, got, want)


@pytest.mark.parametrize("tag", SC.ERR_TAGS)
def test_compute_errors_sizes(tag):
    for n in SC.ERR_SIZES:
        g, p = SC.errors_inputs(n, tag)
        hold_errors(errors_on_device(g, p), g, p, tag, "n=%d" % n)


@pytest.mark.parametrize("tag", SC.ERR_TAGS)
def test_compute_errors_2d_and_strided_view(tag):
    from mal_amd.evaluate import compute_errors
    g, p = SC.errors_inputs(1025, tag)
    g2, p2 = g[:1023].reshape(33, 31), p[:1023].reshape(33, 31)
    hold_errors(errors_on_device(g2, p2), g2, p2, tag, "33x31")
    tg, tp = torch.from_numpy(g2).to(DEV), torch.from_numpy(p2).to(DEV)
    vg, vp = tg.t()[::2, 1:], tp.t()[::2, 1:]
    assert not vg.is_contiguous() and not vp.is_contiguous()
    hold_errors(compute_errors(vg, vp), g2.T[::2, 1:], p2.T[::2, 1:], tag, "strided view")


@pytest.mark.parametrize("tag", SC.ERR_TAGS)
def test_compute_errors_on_the_thresholds(tag):
    for where in SC.PLACEMENTS:
        g, p = SC.threshold_inputs(tag, where)
        hold_errors(errors_on_device(g, p), g, p, tag, where)
