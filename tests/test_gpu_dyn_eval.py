"""GPU: DynamicDepth's validation metrics (mal_amd.dyn_eval, csrc/mal_dyn_eval.hip) over the case table of
tests/dyn_eval_restated.py (proved admissible on the CPU by tests/test_dyn_eval_cases.py).  Every gate compares with the
reference's arithmetic -- torch's own operators on the device, the restatement in float64, the reference's fixtures -- never
with the code under test:

  1  region bytes == F.interpolate(mask, size).bool() run by torch on the device, bitwise
  2  the exported predictions against the float64 restatement: per case the largest relative distance is at most
     max(1e-6, 1.25 x the largest relative distance of torch's own F.interpolate + clamp on the device from that value)
     (whether they are torch's bits depends on how ATen was compiled: printed, not gated); and EVERY point within the bound
     the number formats give for it (pointwise_bound: the source coordinate's roundings times the local depth range, plus
     16 * 2^-24 of the largest tap) -- torch's own distance cannot serve per point, since at a point it may be zero
  3  the median == torch.median of the kernel's own exported predictions, bitwise; the ratio as torch forms it from it
  4  n_all, n_doj, doj/count, dojpxs, allpxs exact
  5  the kernel's own scaled predictions through the restated compute_depth_errors in float64: a1..a3 bit-equal as float32
     values, the other four within 1e-9 (float64 ground truth) / 1e-5 (float32)
  6  the reference's fixtures end to end: per image a1..a3 equal, everything else (the other four, the ratio, val's aggregated
     lists, whose a1..a3 upstream accumulates in numpy's dtype of the day) within 1e-5 relative; the counts exact
  7  the same bytes for one call, one image per call in reverse order, 2 + 1 and 1 + 2, student and teacher interleaved
  8  two runs bitwise equal
  9  the existing DepthEvaluator's outputs on one of its own cases unchanged after this one ran on the same stream
  10 DynamicDepthValPath's dictionaries equal result()'s
and a captured accumulate follows disparities rewritten between replays."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dyn_eval_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WHOS = ("student", "mono")


@pytest.fixture(scope="module", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


def evaluator(c):
    from mal_amd.dyn_eval import DynamicDepthEvaluator
    return DynamicDepthEvaluator(c["gt"], c["split"], DEV)


def feed(ev, c, groups, export=False):
    """``groups``: [(first, count)] in call order; student and teacher interleaved call by call -> {who: [export dicts]}"""
    dev = {k: c[k].to(DEV) for k in ("disp", "mono_disp", "doj_mask")}
    out = {w: [] for w in WHOS}
    for first, n in groups:
        for w, key in zip(WHOS, ("disp", "mono_disp")):
            out[w].append(ev.accumulate(dev[key][first:first + n], dev["doj_mask"][first:first + n], first, w, c["min_depth"],
                                        c["max_depth"], export=export))
    return out


def points(c, i):
    """-> (mask (h,w) bool over the cropped ground truth, selection of the image's packed slots that are valid points,
    (gh, gw), (y0, x0))"""
    gt, mask, size, org = R.valid_points(c["gt"][i], c["split"])
    sel = torch.from_numpy(mask.reshape(-1)) if c["split"] == "cityscapes" else slice(None)
    return torch.from_numpy(mask), sel, size, org


@pytest.fixture(scope="module")
def runs():
    """every sweep case once through the device (one call per network, exported) and once through the float64 restatement"""
    out = {}
    for name in R.SWEEP_CASES:
        c = R.make_case(name)
        ev = evaluator(c)
        ex = feed(ev, c, [(0, len(c["gt"]))], export=True)
        res = {w: ev.result(w) for w in WHOS}
        per = {w: [] for w in WHOS}
        for w in WHOS:
            off = 0
            for i in range(len(c["gt"])):
                slots = int(ev.offsets[i + 1] - ev.offsets[i])
                _, sel, _, _ = points(c, i)
                per[w].append({k: ex[w][0][k][off:off + slots].cpu()[sel] for k in ("pred", "region", "scaled")})
                off += slots
        out[name] = {"case": c, "ev": ev, "res": res, "per": per, "rows": {w: ev.rows(w).cpu().numpy().copy() for w in WHOS},
                     "ref64": {w: R.evaluate_case(c, w, torch.float64) for w in WHOS},
                     "ref32": {w: R.evaluate_case(c, w, resize="explicit") for w in WHOS}}
    return out


def test_gate1_region_bytes_are_atens_nearest(runs):
    for name, r in runs.items():
        c = r["case"]
        m = c["doj_mask"].to(DEV).float()   # the rule picks an index: the same one for every dtype
        for i in range(len(c["gt"])):
            mask, _, (gh, gw), (y0, x0) = points(c, i)
            want = F.interpolate(m[i:i + 1], [gh, gw])[0, 0].bool().cpu()[y0:y0 + mask.shape[0], x0:x0 + mask.shape[1]][mask]
            for w in WHOS:
                assert torch.equal(r["per"][w][i]["region"].bool(), want), (name, i, w)


def pointwise_bound(c, key, i):
    """Per valid point, how far a float32 evaluation of the rule may lie from the float64 one, from the number formats alone:
      * the source coordinate scale * (dst + 0.5) - 0.5 carries the rounding of (float)in / out, of the product and of the
        difference: at most 4 * 2^-24 * (src + 1) in each axis, and lambda inherits it (src - (int)src is exact);
      * the interpolant is continuous and piecewise linear, so such a shift moves it by at most the shift times the range of
        the depths over the cell and its neighbours (the shift may cross into the next cell);
      * the four taps (float32 constants of disp_to_depth, its product, sum and quotient: 5 * 2^-24 relative), 1 - lambda
        (2 * 2^-24) and the four roundings of the weighted sums: at most 11, taken as 16, * 2^-24 * the largest tap.
    The clamp cannot enlarge a distance.  The gate's per-case comparison with torch's own distance stands beside this."""
    depth = R.disp_to_depth(c[key][i, 0].double(), c["min_depth"], c["max_depth"])
    gt, mask, (gh, gw), (y0, x0) = R.valid_points(c["gt"][i], c["split"])
    ys, xs = np.nonzero(mask)
    shift, spans = 0.0, []
    for n_dst, n_src, pts in ((gh, depth.shape[0], torch.from_numpy(ys + y0)), (gw, depth.shape[1], torch.from_numpy(xs + x0))):
        i0, i1, _, l1 = R.bilinear_taps(n_dst, n_src, torch.float64)
        shift = shift + 4 * 2.0 ** -24 * ((i0.double() + l1)[pts] + 1)
        lo, hi = (i0[pts] - 1).clamp(min=0), (i1[pts] + 1).clamp(max=n_src - 1)
        spans.append([torch.minimum(lo + d, hi) for d in range(4)])
    near = torch.stack([depth[r, q] for r in spans[0] for q in spans[1]])   # (16, n): the cell and its neighbours
    return shift * (near.max(0)[0] - near.min(0)[0]) + 16 * 2.0 ** -24 * near.abs().max(0)[0]


def test_gate2_predictions_against_float64(runs):
    worst, bit_equal, total, tightest = 0.0, 0, 0, 0.0
    for name, r in runs.items():
        c = r["case"]
        for w, key in zip(WHOS, ("disp", "mono_disp")):
            depth = R.disp_to_depth(c[key].to(DEV), c["min_depth"], c["max_depth"])
            dk = dt = 0.0
            for i in range(len(c["gt"])):
                mask, _, (gh, gw), (y0, x0) = points(c, i)
                t = torch.clamp(F.interpolate(depth[i:i + 1], [gh, gw], mode="bilinear", align_corners=False), 1e-3, 80)[0, 0]
                t = t.cpu()[y0:y0 + mask.shape[0], x0:x0 + mask.shape[1]][mask].double()
                ref = r["ref64"][w][i]["pred_first"]
                k = r["per"][w][i]["pred"]
                dk = max(dk, float(((k.double() - ref).abs() / ref).max()))
                use = (k.double() - ref).abs() / pointwise_bound(c, key, i)   # every point, against the formats' own bound
                tightest = max(tightest, float(use.max()))
                assert float(use.max()) <= 1.0, (name, w, i, int(use.argmax()), float(use.max()))
                dt = max(dt, float(((t - ref).abs() / ref).max()))
                bit_equal += int((k.double() == t).sum())
                total += k.numel()
            print("gate 2 %-10s %-7s kernel %.3e torch %.3e" % (name, w, dk, dt))
            worst = max(worst, dk)
            assert dk <= max(1e-6, 1.25 * dt), (name, w, dk, dt)
    print("gate 2: largest relative distance %.3e; largest share of a point's own bound %.3f; %d of %d predictions are torch's bits"
          % (worst, tightest, bit_equal, total))


def test_gate3_median_and_ratio(runs):
    for name, r in runs.items():
        c = r["case"]
        f64 = c["gt"][0].dtype == np.float64
        for w in WHOS:
            for i in range(len(c["gt"])):
                pred = r["per"][w][i]["pred"]
                med = torch.median(pred.to(DEV)).cpu()
                row = r["rows"][w][i]
                assert np.float32(row[17]) == med.numpy() and row[17] == float(med), (name, w, i)
                gt = r["ref32"][w][i]["gt"]
                ratio = torch.median(gt) / med   # as trainer.py:1219 forms it: two 0-dim tensors
                assert ratio.dtype == (torch.float64 if f64 else torch.float32)
                assert row[14] == float(ratio), (name, w, i, row[14], float(ratio))
                # the in-place float32 multiply and the second clamp, on the kernel's own first predictions
                want = pred.clone()
                want *= ratio
                assert torch.equal(r["per"][w][i]["scaled"], torch.clamp(want, min=1e-3, max=80)), (name, w, i)


def test_gate4_counts(runs):
    for name, r in runs.items():
        for w in WHOS:
            ref, res = r["ref32"][w], r["res"][w]
            assert list(res["n_all"]) == [x["n_all"] for x in ref] and list(res["n_doj"]) == [x["n_doj"] for x in ref], (name, w)
            assert res["doj/count"] == sum(x["n_doj"] > 0 for x in ref)
            assert res["dojpxs"] == sum(x["n_doj"] for x in ref) and res["allpxs"] == sum(x["n_all"] for x in ref)
            assert (r["rows"][w][res["n_doj"] == 0, 7:14] == 0).all()


def test_gate5_errors_of_the_kernels_own_predictions(runs):
    worst = {True: 0.0, False: 0.0}
    for name, r in runs.items():
        c = r["case"]
        f64 = c["gt"][0].dtype == np.float64
        tol = 1e-9 if f64 else 1e-5
        for w in WHOS:
            for i in range(len(c["gt"])):
                gt, p = r["ref32"][w][i]["gt"], r["per"][w][i]
                reg = p["region"].bool()
                for sel, lo in ((slice(None), 0), (reg, 7)):
                    if lo and not reg.any():
                        continue
                    want = R.compute_depth_errors(gt[sel], p["scaled"][sel], torch.float64)
                    got = r["rows"][w][i][lo:lo + 7]
                    for k in (4, 5, 6):
                        assert want[k].dtype == torch.float32 and np.float32(got[k]) == want[k].numpy() and got[k] == float(want[k]), (name, w, i, lo, k)
                    for k in range(4):
                        d = abs(got[k] - float(want[k])) / max(abs(float(want[k])), 1e-300)
                        worst[f64] = max(worst[f64], d)
                        assert d <= tol, (name, w, i, lo, k, got[k], float(want[k]))
    print("gate 5: largest relative distance %.3e (float64 ground truth), %.3e (float32)" % (worst[True], worst[False]))


def test_gate5_aggregation_in_image_order(runs):
    for name, r in runs.items():
        for w in WHOS:
            rows, res = r["rows"][w], r["res"][w]
            doj = rows[:, 16] > 0
            for k, m in enumerate(R.METRICS):
                s = 0.0
                for v in rows[:, k]:
                    s += v
                assert res[m] == s / len(rows), (name, w, m)
                s = 0.0
                for v in rows[doj, 7 + k]:
                    s += v
                if doj.any():
                    assert res["doj/" + m] == s / doj.sum(), (name, w, m)
                else:
                    assert np.isnan(res["doj/" + m]) and res["doj/count"] == 0, (name, w, m)   # upstream's 0/0


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_gate6_reference_fixtures_end_to_end(name):
    z = R.load_golden(name)
    c = R.case_of_golden(z)
    ev = evaluator(c)
    n = len(c["gt"])
    feed(ev, c, [(0, n)])
    worst = 0.0

    def close(a, b, what):
        nonlocal worst
        d = abs(a - b) / abs(b)
        worst = max(worst, d)
        assert d <= 1e-5, (name, what, a, b)
    for w, lst in zip(WHOS, ("val/errors", "val/mono_err")):
        res = ev.result(w)
        assert list(res["n_all"]) == list(z["n_all"]) and list(res["n_doj"]) == list(z["n_doj"])
        assert (res["doj/count"], res["dojpxs"], res["allpxs"]) == (float(z["val/doj_count"]), int(z["val/dojpxs"]), int(z["val/allpxs"]))
        for i in range(n):
            close(res["ratios"][i], float(z["ratio/%s/%d" % (w, i)]), (w, i, "ratio"))
            for key, got in (("errors/%s/%d" % (w, i), res["per_image"][i]), ("doj_errors/%s/%d" % (w, i), res["doj/per_image"][i])):
                if key not in z:
                    assert res["n_doj"][i] == 0 and (got == 0).all()
                    continue
                assert (got[4:] == z[key][4:]).all(), (name, key, got[4:], z[key][4:])
                for k in range(4):
                    close(got[k], z[key][k], (key, k))
        for k, m in enumerate(R.METRICS):
            close(res[m], z[lst][k], (w, m))
            if w == "student":
                close(res["doj/" + m], z["val/doj_err"][k], (w, "doj/" + m))
    print("gate 6 %s: largest relative distance %.3e" % (name, worst))


def test_gate5_split_without_object_pixels_gives_nan_means(runs):
    for w in WHOS:
        res = runs["nodoj"]["res"][w]
        assert res["doj/count"] == 0 and res["dojpxs"] == 0 and res["allpxs"] == 25
        assert all(np.isnan(res["doj/" + m]) and np.isfinite(res[m]) for m in R.METRICS)
        assert (res["doj/per_image"] == 0).all()


def test_gate7_grouping_and_order(runs):
    for name, r in runs.items():
        c = r["case"]
        if len(c["gt"]) != 3:
            continue
        for groups in ([(2, 1), (1, 1), (0, 1)], [(0, 2), (2, 1)], [(0, 1), (1, 2)], [(1, 2), (0, 1)]):
            ev = evaluator(c)
            feed(ev, c, groups)
            for w in WHOS:
                assert ev.rows(w).cpu().numpy().tobytes() == r["rows"][w].tobytes(), (name, groups, w)


def test_gate8_two_runs_bitwise_equal(runs):
    for name, r in runs.items():
        ev = r["ev"]
        ev.reset()
        ex = feed(ev, r["case"], [(0, len(r["case"]["gt"]))], export=True)
        for w in WHOS:
            assert ev.rows(w).cpu().numpy().tobytes() == r["rows"][w].tobytes(), (name, w)
            off = 0
            for i, p in enumerate(r["per"][w]):
                slots = int(ev.offsets[i + 1] - ev.offsets[i])
                _, sel, _, _ = points(r["case"], i)
                for k in ("pred", "region", "scaled"):
                    assert torch.equal(ex[w][0][k][off:off + slots].cpu()[sel], p[k]), (name, w, i, k)
                off += slots


def test_gate9_existing_evaluator_unchanged(runs):
    from mal_amd.evaluate import DepthEvaluator
    from tests.test_eval_oracle import eigen_inputs
    gts, disp, mono = eigen_inputs(5, True)

    def old():
        ev = DepthEvaluator(gts, "eigen", DEV)
        ev.accumulate(torch.from_numpy(disp).to(DEV), 0, "student")
        ev.accumulate(torch.from_numpy(mono).to(DEV), 0, "mono", disp_max=100.0)
        return [x.tobytes() for w in WHOS for x in ev.result(w)]
    before = old()
    r = runs["eigen1024"]
    r["ev"].reset()
    feed(r["ev"], r["case"], [(0, 3)])
    assert old() == before
    assert r["ev"].rows("student").cpu().numpy().tobytes() == r["rows"]["student"].tobytes()


# dynamicdepth/trainer.py:253-254: the keys Trainer.val creates (:761-775), compute_depth_losses fills (:1243-1256) and val's
# tail divides and reads back (:881-899)
UPSTREAM_NAMES = ["de/abs_rel", "de/sq_rel", "de/rms", "de/log_rms", "da/a1", "da/a2", "da/a3"]


class _Val:
    depth_metric_names = UPSTREAM_NAMES

    def __init__(self, ev, opt):
        self.dyn_evaluator, self.opt = ev, opt


def vals_dictionary(names):
    """what Trainer.val creates before its loop (:760-775)"""
    losses = {}
    for i, metric in enumerate(names):
        losses[metric] = 0.0
        losses['doj/' + metric] = 0.0
    losses['doj/count'] = 0.0
    losses['dojpxs'] = 0
    losses['allpxs'] = 0
    return losses


def test_gate10_mixin_fills_upstreams_dictionaries(runs):
    from types import SimpleNamespace

    from mal_amd.dyn_eval import DynamicDepthValPath

    class Val(DynamicDepthValPath, _Val):
        pass
    names = UPSTREAM_NAMES
    keys = set(vals_dictionary(names))
    for name in ("up12x20", "city3"):
        r = runs[name]
        c = r["case"]
        mask = c["doj_mask"].to(DEV)

        def batch(first, n):
            return ({"doj_mask": mask[first:first + n]},
                    {("disp", 0): c["disp"].to(DEV)[first:first + n], ("mono_disp", 0): c["mono_disp"].to(DEV)[first:first + n]})
        for step in (1, 3):
            ev = evaluator(c)
            val = Val(ev, SimpleNamespace(min_depth=c["min_depth"], max_depth=c["max_depth"]))
            losses, mono_losses = vals_dictionary(names), vals_dictionary(names)
            total_batches = 0
            for first in range(0, 3, step):
                total_batches += step   # upstream: one image per batch
                inputs, outputs = batch(first, step)
                val.compute_depth_losses(inputs, outputs, losses, mono_losses, first, True, accumulate=True)
                assert inputs["doj_mask"].shape == (step, 1) + tuple(mask.shape[2:])   # not overwritten
            assert set(losses) == keys and set(mono_losses) == keys   # no key beside upstream's
            for i, metric in enumerate(names):   # val's tail as written (:881-886)
                losses[metric] /= total_batches
                losses['doj/' + metric] /= losses['doj/count']
                mono_losses[metric] /= total_batches
                mono_losses['doj/' + metric] /= losses['doj/count']
            for w, d in zip(WHOS, (losses, mono_losses)):
                res = r["res"][w]
                for short, metric in zip(R.METRICS, names):
                    assert d[metric] == res[short] and d["doj/" + metric] == res["doj/" + short], (name, step, w, metric)
            assert (losses["doj/count"], losses["dojpxs"], losses["allpxs"]) == tuple(r["res"]["student"][k] for k in ("doj/count", "dojpxs", "allpxs"))
            assert mono_losses["dojpxs"] == 0 and mono_losses["doj/count"] == 0   # upstream counts in ``losses`` alone
        # accumulate=False: the one image's metrics are set, the counts still added (:1231-1241 stand outside the branch)
        one, one_mono = vals_dictionary(names), vals_dictionary(names)
        inputs, outputs = batch(1, 1)
        val.compute_depth_losses(inputs, outputs, one, one_mono, 1, True)
        assert [one[m] for m in names] == list(r["res"]["student"]["per_image"][1]) and set(one) == keys
        assert [one_mono[m] for m in names] == list(r["res"]["mono"]["per_image"][1])
        assert (one["allpxs"], one["dojpxs"], one["doj/count"]) == (r["res"]["student"]["n_all"][1], 0, 0.0)
        assert all(one["doj/" + m] == 0.0 for m in names)
        with pytest.raises(ValueError, match="ONE image"):
            val.compute_depth_losses(*batch(0, 3), one, one_mono, 0, True)
        with pytest.raises(KeyError):   # dictionaries without upstream's keys fail as upstream's own lines do
            val.compute_depth_losses(*batch(1, 1), {m: 0.0 for m in R.METRICS}, {}, 1, False, accumulate=True)


def test_graph_capture_follows_rewritten_disparities(runs):
    r = runs["eigen1024"]
    c = r["case"]
    ev = evaluator(c)
    disp, mask = c["disp"].to(DEV).clone(), c["doj_mask"].to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        ev.accumulate(disp, mask, 0, "student", c["min_depth"], c["max_depth"])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.accumulate(disp, mask, 0, "student", c["min_depth"], c["max_depth"])
    for key, w in (("mono_disp", "mono"), ("disp", "student")):
        disp.copy_(c[key].to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert ev.rows("student").cpu().numpy().tobytes() == r["rows"][w].tobytes(), key
