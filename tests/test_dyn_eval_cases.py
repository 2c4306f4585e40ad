"""CPU: DynamicDepth's validation rule restated (tests/dyn_eval_restated.py) against the reference's own numbers
(tests/golden/dyn_eval_*.npz, scripts/gen_golden_dyn_eval.py) bit for bit, its pieces against torch, the admissibility and the
named properties of the case table tests/test_gpu_dyn_eval.py sweeps, the new symbols and the refusals (no device needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dyn_eval_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


ATEN_NOTE = ("the float32 restatement resizes with F.interpolate itself (tests/dyn_eval_restated.py says why), so this compares "
             "ATen's CPU kernel of THIS torch build with the one that generated the fixture: if no project file changed, a torch "
             "build that vectorises or contracts differently moved these bits -- regenerate with scripts/gen_golden_dyn_eval.py "
             "and check test_written_out_bilinear_is_aten_up_to_its_contractions")


def bits(x):
    a = np.ascontiguousarray(x.detach().numpy() if isinstance(x, torch.Tensor) else x)
    return a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])


def widened(xs):
    return np.array([float(x) for x in xs], np.float64)   # float32 values widen exactly


@pytest.fixture(scope="module")
def sweep():
    """every sweep case with its float32 evaluation (both resize forms), computed once"""
    out = {}
    for name in R.SWEEP_CASES:
        c = R.make_case(name)
        out[name] = (c, {(w, rs): R.evaluate_case(c, w, resize=rs) for w in ("student", "mono") for rs in ("aten", "explicit")})
    return out


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_restatement_equals_the_reference_bit_for_bit(name):
    z = R.load_golden(name)
    c = R.case_of_golden(z)
    made = R.make_case(name, R.GOLDEN_CASES)   # the stored inputs are the table's
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(c["gt"], made["gt"]))
    assert torch.equal(c["disp"], made["disp"]) and torch.equal(c["doj_mask"], made["doj_mask"])
    n = len(c["gt"])
    assert int(z["val/doj_count"]) < n   # one image has no object pixel inside the mask
    for who in ("student", "mono"):
        res = R.evaluate_case(c, who)
        assert [r["n_all"] for r in res] == list(z["n_all"]) and [r["n_doj"] for r in res] == list(z["n_doj"])
        for i, r in enumerate(res):
            assert np.array_equal(bits(r["mask"]), bits(z["mask/%d" % i])) and np.array_equal(bits(r["doj_mask"]), bits(z["doj_mask/%d" % i]))
            assert np.array_equal(bits(r["pred_first"]), bits(z["pred_pts/%s/%d" % (who, i)])), (who, i, ATEN_NOTE)
            assert np.array_equal(bits(r["pred"]), bits(z["scaled_pts/%s/%d" % (who, i)])), (who, i)
            assert r["ratio"].numpy().dtype == z["ratio/%s/%d" % (who, i)].dtype
            assert np.array_equal(bits(r["ratio"]), bits(z["ratio/%s/%d" % (who, i)]))
            assert np.array_equal(bits(r["median"]), bits(z["median/%s/%d" % (who, i)]))
            assert np.array_equal(bits(widened(r["errors"])), bits(z["errors/%s/%d" % (who, i)])), (who, i)
            if r["n_doj"]:
                assert np.array_equal(bits(widened(r["doj_errors"])), bits(z["doj_errors/%s/%d" % (who, i)])), (who, i)
            else:
                assert r["doj_errors"] is None and "doj_errors/%s/%d" % (who, i) not in z
            key = "pred_full/%s/%d" % (who, i)
            if key in z:
                assert np.array_equal(bits(r["pred_full"]), bits(z[key])), (who, i, ATEN_NOTE)
        # val's tail: upstream accumulates a1..a3 in numpy's promoted dtype of its version; the restatement in float64
        agg = R.aggregate(res)
        for lst, pre in ((z["val/errors"] if who == "student" else z["val/mono_err"], ""),) + (
                ((z["val/doj_err"], "doj/"),) if who == "student" else ()):
            for m, v in zip(R.METRICS, lst):
                assert abs(v - agg[pre + m]) <= 1e-6 * abs(v), (who, pre + m)
        assert agg["doj/count"] == float(z["val/doj_count"]) and agg["dojpxs"] == int(z["val/dojpxs"]) and agg["allpxs"] == int(z["val/allpxs"])
    # the even and the odd count
    assert {int(x) % 2 for x in z["n_all"]} == {0, 1}


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 8, 1023, 1024, 1025])
def test_lower_median_is_torch_median_with_ties(n):
    g = torch.Generator().manual_seed(n)
    v = torch.randint(0, max(2, n // 3), (n,), generator=g).float() / 7 + 1   # many ties, also around the middle
    m, i = R.lower_median(v)
    assert torch.equal(m, torch.median(v)) and float(v[i]) == float(m)
    assert float(m) == float(torch.sort(v)[0][(n - 1) // 2])
    if n % 2 == 0 and n > 2:
        w = torch.arange(n, dtype=torch.float64)
        assert float(R.lower_median(w)[0]) == float(torch.median(w)) == n // 2 - 1 != float(np.median(w.numpy()))


def test_nearest_rule_is_aten_on_the_sweeps_mask_sizes():
    sizes = set()
    for name, t in list(R.SWEEP_CASES.items()) + list(R.GOLDEN_CASES.items()):
        gh, gw = R.valid_points(np.zeros(t[2]), t[0])[2]
        sizes.add((t[4], (gh, gw)))
    assert len(sizes) >= 10
    for (mh, mw), (gh, gw) in sorted(sizes):
        m = torch.arange(mh * mw, dtype=torch.float32).reshape(mh, mw)
        assert torch.equal(R.resize_nearest(m, gh, gw), F.interpolate(m[None, None], [gh, gw])[0, 0]), ((mh, mw), (gh, gw))
        u = (m.to(torch.int64) % 251).to(torch.uint8)
        assert torch.equal(R.resize_nearest(u, gh, gw), F.interpolate(u[None, None], [gh, gw])[0, 0])


def test_written_out_bilinear_is_aten_up_to_its_contractions():
    """ATen's CPU build fuses multiply-adds the written-out form rounds separately: same taps, so the two differ by a few ulp
    of the largest tap; in float64 they agree to 1e-12.  (Where nothing is interpolated they are equal.)"""
    torch.manual_seed(0)
    for (h, w), (gh, gw) in (((1, 1), (9, 13)), ((1, 7), (9, 13)), ((5, 1), (9, 13)), ((2, 2), (9, 13)), ((6, 10), (6, 10)),
                             ((6, 10), (7, 11)), ((3, 5), (12, 20)), ((24, 64), (93, 310)), ((12, 32), (258, 2048))):
        d = R.disp_to_depth(torch.rand(h, w), 0.1, 100.0)
        a = R.resize_bilinear(d, gh, gw)
        b = F.interpolate(d[None, None], [gh, gw], mode="bilinear", align_corners=False)[0, 0]
        assert float((a - b).abs().max()) <= 64 * 2.0 ** -24 * float(d.max()), ((h, w), (gh, gw))
        if (h, w) == (gh, gw):
            assert torch.equal(a, b)
        a64 = R.resize_bilinear(d.double(), gh, gw)
        b64 = F.interpolate(d.double()[None, None], [gh, gw], mode="bilinear", align_corners=False)[0, 0]
        assert float((a64 - b64).abs().max()) <= 1e-12 * float(d.max())
        assert float((a64 - b.double()).abs().max()) <= 1e-4 * float(d.max())


def test_ratio_is_rounded_to_float32_before_the_multiply():
    """the in-place multiply of a float32 map by a 0-dim float64 tensor (trainer.py:1219): DESIGN.md 19"""
    p = torch.rand(4096) * 50 + 1
    r = torch.tensor(1.2345678901234567, dtype=torch.float64)
    q = p.clone()
    q *= r
    assert q.dtype == torch.float32 and torch.equal(q, p * r.float()) and not torch.equal(q, (p.double() * r).float())


def test_sweep_is_admissible_in_float32_alone(sweep):
    for name, (c, ev) in sweep.items():
        for key, res in ev.items():
            assert min(r["margin"] for r in res) > 1e-4, (name, key)
    for name in R.GOLDEN_CASES:
        c = R.case_of_golden(R.load_golden(name))
        assert R.admissible(c), name
        # ... so ATen's contracted resize (the fixtures) and the separately rounded one (the device) take the same comparisons
        for w in ("student", "mono"):
            for a, b in zip(R.evaluate_case(c, w, resize="aten"), R.evaluate_case(c, w, resize="explicit")):
                assert [float(x) for x in a["errors"][4:]] == [float(x) for x in b["errors"][4:]], (name, w)


def test_sweep_covers_what_the_issue_lists(sweep):
    t = R.SWEEP_CASES
    assert {(v[1], v[2]) for v in t.values()} >= {((1, 1), (9, 13)), ((1, 7), (9, 13)), ((5, 1), (9, 13)), ((2, 2), (9, 13)),
                                                  ((6, 10), (6, 10)), ((6, 10), (7, 11)), ((3, 5), (12, 20)), ((24, 64), (93, 310))}
    counts = {r["n_all"] for c, ev in sweep.values() for r in ev[("student", "aten")]}
    assert counts >= {1, 2, 3, 4, 1023, 1024, 1025, 2049}
    assert {v[3] for v in t.values()} == {"f4", "f8"} and {v[5] for v in t.values()} == {"f4", "u1"}
    assert {len(v[6]) for v in t.values()} == {1, 3}
    assert any(v[4] == v[1] for v in t.values()) and any(v[4] != v[1] for v in t.values())
    # dense windows of 2 and 3 rows of 1664 slots
    for name, rows in (("city2", 2), ("city3", 3)):
        g, m, (gh, gw), (y0, x0) = R.valid_points(sweep[name][0]["gt"][0], "cityscapes")
        assert g.shape == (rows, 1664) and (y0, x0) == (256, 192) and gw == 2048


def test_named_cases_have_their_property(sweep):
    # a source coordinate clamped by max(0, .) in a column, and a second tap clamped in a row and in a column
    def taps_hit(name):
        c = sweep[name][0]
        t = R.SWEEP_CASES[name]
        hit = {"col0": False, "row_last": False, "col_last": False}
        for g in c["gt"]:
            gt, mask, (gh, gw), (y0, x0) = R.valid_points(g, t[0])
            ys, xs = np.nonzero(mask)
            ys, xs = ys + y0, xs + x0
            for n_dst, n_src, pts, keys in ((gw, t[1][1], xs, ("col0", "col_last")), (gh, t[1][0], ys, (None, "row_last"))):
                scale = np.float32(n_src) / np.float32(n_dst)
                raw = scale * (pts.astype(np.float32) + np.float32(0.5)) - np.float32(0.5)
                if keys[0] and n_src > 1 and (raw < 0).any():
                    hit[keys[0]] = True
                if (np.maximum(raw, 0).astype(np.int64) >= n_src - 1).any():
                    hit[keys[1]] = True
        return hit
    assert taps_hit("up12x20")["col0"] and taps_hit("d2x2")["col0"]
    assert taps_hit("d1x7")["row_last"] and taps_hit("d5x1")["col_last"] and taps_hit("up12x20")["row_last"]
    # a point clamped at 1e-3 and one at 80, before and after scaling
    res = sweep["clamps"][1][("student", "aten")]
    first = torch.cat([r["pred_first"] for r in res])
    assert (first == 80).any() and (first == torch.tensor(1e-3)).any()
    assert any(((r["pred"] == 80) & (r["pred_first"] < 80)).any() for r in res)
    assert any(((r["pred"] == torch.tensor(1e-3)) & (r["pred_first"] > torch.tensor(1e-3))).any() for r in res)
    # an image with n_doj == 0 and one whose object region is the whole mask, in every three-image case
    for name, (c, ev) in sweep.items():
        res = ev[("student", "aten")]
        if len(res) == 3:
            assert res[1]["n_doj"] == 0 and res[2]["n_doj"] == res[2]["n_all"] and 0 < res[0]["n_doj"], name
    # one image without any object pixel: doj/count == 0, the aggregation's 0/0
    (r,) = sweep["nodoj"][1][("student", "aten")]
    assert r["n_doj"] == 0 and r["n_all"] > 0 and np.isnan(R.aggregate([r])["doj/abs_rel"])
    # tied predictions around the median, on an even count
    r = sweep["eigen1024"][1][("student", "aten")][1]
    assert r["n_all"] % 2 == 0 and len(torch.unique(r["pred_first"])) < r["n_all"]
    # ulps6x10: an odd count, an even count and all predictions equal; each image's predictions are its own pixels' depths,
    # share their top 24 bits (the first two passes of the 12 + 12 + 8 bit select see one bin) and the median is the lower
    # middle value, which on the even count is not the upper one
    c, ev = sweep["ulps6x10"]
    for (w, rs), res in ev.items():
        assert [r["n_all"] % 2 for r in res[:2]] == [1, 0], (w, rs)
        depth = R.disp_to_depth(c["disp" if w == "student" else "mono_disp"], c["min_depth"], c["max_depth"])
        for i, r in enumerate(res):
            p, n = r["pred_first"], r["n_all"]
            assert torch.equal(p, depth[i, 0][r["mask"]]), (w, rs, i)   # taps (1, 0), no clamp
            assert len(np.unique(bits(p) >> 8)) == 1 and len(np.unique(bits(p))) == (1 if i == 2 else n), (w, rs, i)
            order = torch.sort(p)[0]
            assert float(p[r["median_index"]]) == float(order[(n - 1) // 2]) == float(r["median"]), (w, rs, i)
        assert res[1]["median"] < torch.sort(res[1]["pred_first"])[0][res[1]["n_all"] // 2], (w, rs)
        assert res[2]["median_index"] == (res[2]["n_all"] - 1) // 2, (w, rs)   # all equal: the stable order's middle


def test_each_variant_moves_a_case(sweep):
    """the one-edit departures the device file is tried with, on the restatement: each changes what a gate of
    tests/test_gpu_dyn_eval.py compares in at least one sweep case"""
    moved = {v: [] for v in ("upper", "mean2", "noclamp1", "nearest_half", "lam_before_max")}
    for name, (c, ev) in sweep.items():
        base = ev[("student", "explicit")]
        for v in moved:
            res = R.evaluate_case(c, "student", variant=v, resize="explicit")
            if any(not torch.equal(a["pred_first"], b["pred_first"]) or a["n_doj"] != b["n_doj"] or
                   float(a["median"]) != float(b["median"]) for a, b in zip(res, base)):
                moved[v].append(name)
    assert all(moved.values()), moved


def test_forced_decisions(sweep):
    """the forced form: the restatement's OWN decisions forced on it change nothing, in float32 and float64, for both regions;
    another median position or a flipped comparison changes exactly what it should"""
    for name in ("up12x20", "eigen1024", "city2", "nodoj"):
        c, ev = sweep[name]
        for dtype, base in ((torch.float32, ev[("student", "explicit")]), (torch.float64, R.evaluate_case(c, "student", torch.float64))):
            forced = []
            for r in base:
                th = torch.max(r["gt"] / r["pred"], r["pred"] / r["gt"])
                forced.append({"median_index": r["median_index"], "lt": [th < t for t in R.THRESHOLDS]})
            again = R.evaluate_case(c, "student", dtype, forced=forced, resize="explicit")
            for a, b in zip(again, base):
                assert torch.equal(a["pred"], b["pred"]) and torch.equal(a["ratio"], b["ratio"]) and a["median_index"] == b["median_index"]
                assert [float(x) for x in a["errors"]] == [float(x) for x in b["errors"]], (name, dtype)
                assert (a["doj_errors"] is None) == (b["doj_errors"] is None)
                if b["doj_errors"] is not None:
                    assert [float(x) for x in a["doj_errors"]] == [float(x) for x in b["doj_errors"]], (name, dtype)
    c, ev = sweep["up12x20"]
    base = ev[("student", "explicit")]
    r = base[0]
    other = int(torch.argmax(r["pred_first"]))   # the largest prediction taken for the median: a smaller ratio
    th = torch.max(r["gt"] / r["pred"], r["pred"] / r["gt"])
    lt = [th < t for t in R.THRESHOLDS]
    inside = int(torch.nonzero(r["region"])[0])
    lt[0] = lt[0].clone()
    lt[0][inside] = ~lt[0][inside]   # one comparison of a point inside the object region flipped
    moved = R.evaluate_image(c["gt"][0], c["disp"][0, 0], c["doj_mask"][0, 0], c["split"], c["min_depth"], c["max_depth"],
                             forced={"median_index": other}, resize="explicit")
    assert float(moved["median"]) == float(r["pred_first"][other]) > float(r["median"]) and float(moved["ratio"]) < float(r["ratio"])
    flipped = R.evaluate_image(c["gt"][0], c["disp"][0, 0], c["doj_mask"][0, 0], c["split"], c["min_depth"], c["max_depth"],
                               forced={"lt": lt}, resize="explicit")
    sign = 1 if bool(lt[0][inside]) else -1
    assert round((float(flipped["errors"][4]) - float(r["errors"][4])) * r["n_all"]) == sign
    assert round((float(flipped["doj_errors"][4]) - float(r["doj_errors"][4])) * r["n_doj"]) == sign
    assert [float(x) for x in flipped["errors"][:4]] == [float(x) for x in r["errors"][:4]] and float(flipped["errors"][5]) == float(r["errors"][5])


def test_symbols_header_and_binding():
    from mal_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mal_hip.h")).read()
    for sym in ("mal_eval_dyn_accumulate", "mal_eval_dyn_mean"):
        assert re.search(r"\bint %s\(" % sym, header) and sym in _lib.SIGNATURES and hasattr(lib, sym)
    assert "} mal_eval_dyn_args;" in header and "mal_dyn_eval.hip" in build.SOURCES
    assert lib.mal_struct_bytes(11) == C.sizeof(_lib.EvalDynArgs) > 0 and lib.mal_struct_bytes(12) == 0
    assert (_lib.EVAL_DYN_ROW, _lib.EVAL_DYN_MEAN) == tuple(int(re.search(r"#define %s (\d+)" % k, header).group(1))
                                                            for k in ("MAL_EVAL_DYN_ROW", "MAL_EVAL_DYN_MEAN"))
    import mal_amd
    from mal_amd import dyn_eval
    assert mal_amd.DynamicDepthEvaluator is dyn_eval.DynamicDepthEvaluator and mal_amd.DynamicDepthValPath is dyn_eval.DynamicDepthValPath


def test_entry_points_refuse_bad_arguments_without_device():
    from mal_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    fake = 0x1000  # never dereferenced: every check below fails before any HIP call
    good = dict(n_images=4, first=0, B=2, H=8, W=16, mh=8, mw=16, mask_dtype=0, gt_f64=1, min_depth=0.1, max_depth=100.0,
                seg=fake, idx=fake, gt=fake, disp=fake, mask=fake, pred=fake, region=fake, scaled=None, img_out=fake, stream=None)
    assert lib.mal_eval_dyn_accumulate(None) == -1
    for kw in (dict(seg=None), dict(gt=None), dict(disp=None), dict(mask=None), dict(pred=None), dict(region=None),
               dict(img_out=None), dict(n_images=0), dict(B=0), dict(first=-1), dict(first=3), dict(B=5), dict(H=0), dict(W=0),
               dict(mh=0), dict(mw=0), dict(mask_dtype=2), dict(mask_dtype=-1), dict(min_depth=0.0), dict(max_depth=0.05)):
        a = _lib.EvalDynArgs(**dict(good, **kw))
        assert lib.mal_eval_dyn_accumulate(C.byref(a)) == -1, kw
    assert lib.mal_eval_dyn_mean(None, 4, fake, None) == -1
    assert lib.mal_eval_dyn_mean(fake, 4, None, None) == -1
    assert lib.mal_eval_dyn_mean(fake, 0, fake, None) == -1


def test_evaluator_refusals_without_device():
    from mal_amd import _lib
    from mal_amd.dyn_eval import DynamicDepthEvaluator
    c = R.make_case("up12x20")
    with pytest.raises(_lib.MalError, match="no CPU path"):
        DynamicDepthEvaluator(c["gt"], "eigen", device="cpu")
    for split in ("kitti", "eigen_improved", None):
        with pytest.raises(ValueError, match="eval_split"):
            DynamicDepthEvaluator(c["gt"], split, device="cpu")
    empty = np.zeros_like(c["gt"][1])
    empty[0, 0] = 5.0   # outside the crop
    with pytest.raises(ValueError, match="image 1 has no valid"):
        DynamicDepthEvaluator([c["gt"][0], empty], "eigen", device="cpu")
    with pytest.raises(ValueError, match="literals"):
        DynamicDepthEvaluator(c["gt"], "eigen", device="cpu", max_depth=100)
