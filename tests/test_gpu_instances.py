"""GPU: mal_amd.instances (mal_instances: three HIP launches) against the reference's own outputs
(tests/golden/instances_*.npz, written by scripts/gen_golden_instances.py), the fp64 checker tests/instances_restated.py
and upstream's tail restated with torch operators on the device (instances_restated.torch_tail).

Gates.  Mask bytes, classes, query indices and counts are integers and must be EQUAL: the fixtures' mask logits are
multiples of 1/256, so every upsampled value is exact in fp32 in any order, and their selections have margins >= 1e-5.
cls_score, mask_score and score are compared with the checker's fp64 values: relative distance <= max(1.25 x the
reference's own fp32 distance stored in the fixture, 1e-6); the floor covers a few ulp of exp in the softmax and the
sigmoid plus the final roundings (measured distances: DESIGN.md, "Instances").  The sweep against torch compares
selections as sets and bytes for equality; its scores are two fp32 evaluations of the same quantity, each a few ulp from
the truth, and are held to 4e-6 relative (twice the fixtures' gate for two such distances, the second one torch's, whose
fp32 sums over up to 122880 pixels are not the fixtures' few hundred)."""
import functools

import numpy as np
import pytest
import torch

from tests import instances_restated as R
from tests import matcher_restated as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 1e-6


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(logits, planes, H, W, T, thing=None):
    """(N,Q,K+1), (N,Q,h,w) numpy -> per image a dict of numpy arrays"""
    from mal_amd.instances import instance_inference
    out = instance_inference(dev(logits), dev(planes), (H, W), topk=T, thing_classes=None if thing is None else dev(thing))
    res = []
    for o in out:
        i = o["instances"]
        assert i.pred_masks.dtype == torch.uint8 and i.pred_masks.is_cuda and i.pred_classes.dtype == torch.int64
        assert i.image_size == (H, W) and tuple(i.pred_masks.shape) == (len(i), H, W)
        res.append({k: getattr(i, k).cpu().numpy() for k in ("pred_masks", "scores", "pred_classes", "query", "cls_score",
                                                             "mask_score")})
    return res


@functools.lru_cache(maxsize=None)
def case(tag):
    return R.load_case(tag)


@pytest.mark.parametrize("tag", list(R.CASES))
def test_fixture_cases(tag):
    d = case(tag)
    K = d["K"]
    args = (d["logits"][None], d["planes"][None], d["H"], d["W"], d["T"], d["thing"])
    (o,), (again,) = run(*args), run(*args)
    c = R.checker(d["logits"], d["planes"], d["H"], d["W"], d["T"], d["thing"])
    assert len(o["pred_classes"]) == len(d["ref_flat"])  # count
    assert np.array_equal(o["query"], c["query"]) and np.array_equal(o["pred_classes"], c["classes"])  # the defined order
    at = {f: k for k, f in enumerate(d["ref_flat"].tolist())}
    rows = np.array([at[f] for f in (o["query"].astype(np.int64) * K + o["pred_classes"]).tolist()], dtype=np.int64)
    assert set(np.unique(o["pred_masks"]).tolist()) <= {0, 1}
    assert np.array_equal(o["pred_masks"].astype(bool), d["ref_masks"][rows])  # the reference's bytes, no exemptions
    dist = {k: R.rel_dist(o[mine], d[k]) for k, mine in (("cls_score", "cls_score"), ("mask_score", "mask_score"), ("score", "scores"))}
    print("case %s: count %d, kernel distance from fp64 cls %.3g mask %.3g score %.3g (reference's %.3g %.3g %.3g)"
          % ((tag, len(rows), dist["cls_score"], dist["mask_score"], dist["score"]) + tuple(d["ref_dist"])))
    for k, ref in zip(("cls_score", "mask_score", "score"), d["ref_dist"]):
        assert dist[k] <= max(1.25 * ref, FLOOR), k
    for k in o:  # a second call: the same bits
        assert o[k].tobytes() == again[k].tobytes(), k


def test_case_e_filter_that_keeps_nothing():
    d = case("e")
    z = np.load(R.GOLDEN + "/instances_e.npz")
    (o,) = run(d["logits"][None], d["planes"][None], d["H"], d["W"], d["T"], z["alt_thing"])
    assert int(z["alt_count"]) == 0 and len(o["pred_classes"]) == 0 and o["pred_masks"].shape == (0, d["H"], d["W"])
    # and in a batch with an image that keeps everything: the counts are per image
    thing = np.zeros(d["K"], dtype=bool)
    thing[:6] = True
    both = run(np.stack([d["logits"], d["logits"][::-1]]), np.stack([d["planes"], d["planes"][::-1]]), d["H"], d["W"], d["T"], thing)
    assert len(both[0]["pred_classes"]) == 6 and len(both[1]["pred_classes"]) == 6
    assert np.array_equal(both[0]["pred_masks"].astype(bool), R.checker(d["logits"], d["planes"], d["H"], d["W"], d["T"])["masks"])


@functools.lru_cache(maxsize=None)
def sweep_inputs(N, Q, K, h, w, T):
    """seeded dyadic mask logits; class logits whose selection has a margin (found on the CPU, fp64)"""
    rng = np.random.default_rng(7 + 13 * N + Q + 1000 * h + w)
    planes = rng.integers(-16 * R.MASK_UNIT, 16 * R.MASK_UNIT + 1, (N, Q, h, w)).astype(np.float32) / R.MASK_UNIT
    logits = np.empty((N, Q, K + 1), dtype=np.float32)
    for n in range(N):
        for _ in range(100):
            logits[n] = (rng.standard_normal((Q, K + 1)) * 2.0).astype(np.float32)
            s = np.sort(R.class_scores(logits[n]))[::-1]
            if T == len(s) or (s[T - 1] - s[T]) / s[T - 1] >= 1e-5:
                break
        else:
            raise AssertionError("no class logits with a margin at the cut")
    return logits, planes


@pytest.mark.parametrize("Q", [1, 100])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 2, 3, 5), (2, 3, 8, 12), (5, 17, 20, 65), (48, 160, 192, 640)],
                         ids=lambda s: "x".join(map(str, s)))
def test_sweep_against_torch_on_the_device(shape, N, Q):
    from mal_amd.instances import instance_inference
    h, w, H, W = shape
    K = 8
    T = min(Q * K, 100) if Q > 1 else 5
    thing = np.array([1, 1, 0, 1, 1, 1, 0, 1], dtype=bool) if N == 3 else None
    logits, planes = sweep_inputs(N, Q, K, h, w, T)
    lg, pm = dev(logits), dev(planes)
    theirs = R.torch_tail(lg, pm, H, W, T, thing)
    mine = instance_inference(lg, pm, (H, W), topk=T, thing_classes=None if thing is None else dev(thing))
    worst = 0.0
    for n in range(N):
        i, t = mine[n]["instances"], theirs[n]
        flat = i.query.long() * K + i.pred_classes
        a, b = torch.argsort(flat), torch.argsort(t["flat"])
        assert torch.equal(flat[a], t["flat"][b])  # the same (query, class) pairs, as sets
        assert len(flat) == (T if thing is None else int(thing[(t["flat"] % K).cpu().numpy()].sum()))
        assert torch.equal(i.pred_masks[a], t["masks"][b].to(torch.uint8))  # bytes equal
        assert bool((i.cls_score[:-1] >= i.cls_score[1:]).all())  # descending
        if len(flat):
            rel = ((i.scores[a] - t["scores"][b]).abs() / t["scores"][b].abs().clamp_min(1e-30))[t["scores"][b] != 0]
            worst = max(worst, float(rel.max()) if rel.numel() else 0.0)
            assert bool((i.scores[a][t["scores"][b] == 0] == 0).all())
    print("sweep %s N=%d Q=%d: largest relative score distance from torch's fp32 %.3g" % (shape, N, Q, worst))
    assert worst <= 4e-6


@pytest.mark.parametrize("Q,K,T", [(128, 8, 100), (129, 8, 100), (200, 80, 128), (2048, 8, 128), (16, 1024, 64)],
                         ids=lambda v: str(v))
def test_selection_sizes(Q, K, T):
    """Q*K on both sides of 1024, where the selection goes from 256 threads x 4 candidates to 1024 x 16, at the stated
    bounds (Q*K = 16384, K + 1 = 1025) and at upstream's largest configuration (Q=200, K=80), against the fp64 checker"""
    h, w, H, W = 2, 3, 7, 11
    logits, planes = sweep_inputs(2, Q, K, h, w, T)
    out = run(logits, planes, H, W, T)
    for n in range(2):
        c = R.checker(logits[n], planes[n], H, W, T)
        assert c["margin_sel"] > 0  # (no two selected fp64 scores are equal; the cut has its margin from sweep_inputs)
        o = out[n]
        same = np.array_equal(o["query"], c["query"]) and np.array_equal(o["pred_classes"], c["classes"])
        if not same:  # two fp64 scores that round to one fp32 value change places: the sets must still agree
            close = np.abs(np.diff(c["cls_score"])) <= 2.0 ** -23 * c["cls_score"][:-1]
            assert close.any() and sorted((o["query"].astype(np.int64) * K + o["pred_classes"]).tolist()) == sorted(c["flat"].tolist())
            continue
        assert np.array_equal(o["pred_masks"].astype(bool), c["masks"])
        for mine, k in (("cls_score", "cls_score"), ("mask_score", "mask_score"), ("scores", "score")):
            assert R.rel_dist(o[mine], c[k]) <= FLOOR, k


def test_exact_ties_go_to_the_lower_flat_index():
    """equal logits give equal scores to the bit: the order is the defined one, ascending q*K + c within a score; torch's
    topk(sorted=False) has no order to compare with, the fp64 checker states the rule"""
    Q, K, h, w, H, W = 20, 8, 2, 3, 8, 12
    rng = np.random.default_rng(3)
    planes = rng.integers(-16 * R.MASK_UNIT, 16 * R.MASK_UNIT + 1, (3, Q, h, w)).astype(np.float32) / R.MASK_UNIT
    logits = np.zeros((3, Q, K + 1), dtype=np.float32)  # image 0: every score equal
    logits[1, 5:9] = 1.0                                # image 1: still every score equal (softmax of a constant row)
    logits[2, ::2, :K:3] = 2.0                          # image 2: two levels, the cut falls inside the lower one
    logits[2, 7, 2] = 2.0
    for T in (10, 64, 128):
        out = run(logits, planes, H, W, T)
        for n in range(3):
            c = R.checker(logits[n], planes[n], H, W, T)
            assert c["margin_sel"] == 0  # ties among the selected, as intended
            assert np.array_equal(out[n]["query"], c["query"]) and np.array_equal(out[n]["pred_classes"], c["classes"]), (T, n)
            assert np.array_equal(out[n]["pred_masks"].astype(bool), c["masks"])
        assert np.array_equal(out[0]["query"].astype(np.int64) * K + out[0]["pred_classes"], np.arange(T))


def test_general_fp32_logits():
    """N(0, 4) mask logits, nothing dyadic: a byte may differ from the fp64 rule only where |fp64 value| <= 4 x 2^-23 x the
    largest tap magnitude (the fp32 rounding of three multiply-adds), and such pixels are at most 1e-5 of all"""
    logits, planes = R.general_inputs()
    H, W, T = 192, 640, 100
    (o,) = run(logits[None], planes[None], H, W, T)
    flat = R.select(R.class_scores(logits), T)
    assert np.array_equal(o["query"], flat // 8) and np.array_equal(o["pred_classes"], flat % 8)
    outside, differ, inside = R.band_report(o["pred_masks"], planes[o["query"]], H, W)
    print("general case: %d of %d pixels differ from the fp64 rule (%d outside the band), %d inside the band"
          % (differ, T * H * W, outside, inside))
    assert outside == 0 and differ <= 1e-5 * T * H * W


# ---- integration: InstanceSegmenter + HungarianMatcher drive dyn_utils.image_synthesis ------------------------------------

def stub_planes(h, w, b, frame):
    """three instances as mask logits +-8 on 1/4-resolution ellipses; frame -1 / +1 (the warped frames) shows them moved by
    one texel = four pixels to the left / right of frame 0 (the target); two more queries see nothing"""
    cy = [int(h * f) + (b if h > 8 else 0) for f in (0.35, 0.55, 0.4)]
    cx = [int(w * f) + frame for f in (0.2, 0.5, 0.8)]
    ry, rx = max(1, int(h * 0.22)), max(1, int(w * 0.1))
    inside = MR.ellipse_masks([[y, x, ry, rx] for y, x in zip(cy, cx)], h, w)
    planes = np.full((5, h, w), -8.0, dtype=np.float32)
    planes[:3][inside] = 8.0
    return planes


def stub_logits():
    """class logits peaked by +12 (and a little more, so that the order of the three is not a matter of rounding) on the
    classes 1, 3, 0; the two empty queries are peaked on "no object" """
    logits = np.zeros((5, 5), dtype=np.float32)
    logits[0, 1], logits[1, 3], logits[2, 0] = 12.0, 12.5, 13.0
    logits[3:, 4] = 12.0
    return logits


class StubNet(torch.nn.Module):
    """the segmenter network's place: the first call sees the B target frames, every later call the two warped frames of
    the next sample"""

    def __init__(self, B):
        super().__init__()
        self.B, self.calls, self.shapes = B, 0, []

    def forward(self, x):
        h, w = x.shape[2] // 4, x.shape[3] // 4
        self.shapes.append(tuple(x.shape))
        if self.calls == 0:
            planes = [stub_planes(h, w, b, 0) for b in range(self.B)]
        else:
            planes = [stub_planes(h, w, self.calls - 1, -1), stub_planes(h, w, self.calls - 1, 1)]
        self.calls += 1
        assert x.shape[0] == len(planes)
        return {"pred_logits": dev(np.stack([stub_logits()] * len(planes))), "pred_masks": dev(np.stack(planes))}


@pytest.mark.parametrize("size", [(24, 40), (192, 640)], ids=lambda s: "x".join(map(str, s)))
def test_segmenter_and_matcher_drive_image_synthesis(size):
    from mal_amd import dyn_utils
    from mal_amd.instances import Instances, InstanceSegmenter
    from mal_amd.matcher import HungarianMatcher
    B, (H, W) = 2, size
    mean, std = [103.53, 116.28, 123.675], [57.375, 57.12, 58.395]
    g = torch.Generator().manual_seed(11)
    color = {f: torch.rand(B, 3, H, W, generator=g).to(DEV) for f in (-1, 0, 1)}
    wl, wn = torch.rand(B, 3, H, W, generator=g).to(DEV), torch.rand(B, 3, H, W, generator=g).to(DEV)
    # 24x40 is no multiple of 32: a plane padded by more than three pixels is outside the supported crop, pad to 8 there
    div = 32 if H % 32 == 0 and W % 32 == 0 else 8

    def library_segmenter():
        return InstanceSegmenter(StubNet(B), mean, std, size_divisibility=div, topk=3)

    def restated_segmenter():
        seg = InstanceSegmenter(StubNet(B), mean, std, size_divisibility=div, topk=3)

        def ins_model(images):
            out = seg.net(seg.preprocess(images))
            res = []
            for t in R.torch_tail(out["pred_logits"], out["pred_masks"], H, W, 3):
                order = torch.argsort(t["cls_score"], descending=True)  # the order this library defines
                res.append({"instances": Instances((H, W), t["masks"][order].to(torch.uint8), t["scores"][order], t["classes"][order])})
            return res
        return ins_model

    def produce(ins_model):
        leaves = {f: color[f].clone().requires_grad_(True) for f in (-1, 1)}
        outputs = {("color", -1, 0): leaves[-1], ("color", 1, 0): leaves[1]}
        seen = []

        def recording(images):
            seen.append(ins_model(images))
            return seen[-1]

        has_ins = dyn_utils.image_synthesis({("color", 0, 0): color[0]}, outputs, 0, 0.9, recording, HungarianMatcher())
        assert has_ins is True
        ((outputs[("syn", -1, 0)] * wl).sum() + (outputs[("syn", 1, 0)] * wn).sum()).backward()
        return outputs, leaves, seen

    seg = library_segmenter()
    out_l, leaves_l, seen = produce(seg)
    out_r, leaves_r, _ = produce(restated_segmenter())
    assert seg.net.calls == 1 + B and seg.net.shapes[0] == (B, 3, H, W) and seg.net.shapes[1] == (2, 3, H, W)
    for res in seen:
        for r in res:
            i = r["instances"]
            assert len(i) == 3 and i.pred_classes.tolist() == [0, 3, 1] and i.query.tolist() == [2, 1, 0]
            assert bool(((i.scores - 0.9).abs() > 1e-3).all()) and bool((i.scores > 0.9).all()), i.scores
    for key in (("syn", -1, 0), ("syn", 1, 0), ("syn_region", 0)):
        assert torch.equal(out_l[key], out_r[key]), key
    assert bool((out_l[("syn", -1, 0)] != color[-1]).any())  # the instances moved something
    for f in (-1, 1):
        assert torch.equal(leaves_l[f].grad, leaves_r[f].grad)
