"""GPU: mal_amd.matcher.HungarianMatcher (mal_match: three HIP launches) against the reference's own outputs
(tests/golden/matcher_*.npz, written by scripts/gen_golden_matcher.py) and the CPU checker tests/matcher_restated.py.

Tolerances.  The costs lie in [0, 2); the kernel forms each in fp64 and rounds it once to fp32, whose spacing there is
<= 2.4e-7: |C - fp64 evaluation| <= 2.5e-7 absolute, and so <= 3e-7 against the reference's fp32 matrices.  The pairs
are integers and must be equal: every fixture's optimum is unique by >= 1e-4."""
import functools

import numpy as np
import pytest
import torch

from tests import matcher_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


class _Inst:
    """the slice of detectron2's Instances that the matcher and image_synthesis touch"""

    def __init__(self, classes, masks, scores=None):
        self.pred_classes, self.pred_masks = classes, masks
        self.scores = scores if scores is not None else torch.full((len(classes),), 0.9)

    def __len__(self):
        return len(self.pred_classes)

    def __getitem__(self, sel):
        sel_d = sel.to(self.pred_masks.device) if torch.is_tensor(sel) else sel
        return _Inst(self.pred_classes[sel_d], self.pred_masks[sel_d], self.scores[sel])


@functools.lru_cache(maxsize=None)
def case(tag):
    d = R.load_case(tag)
    d["D1"] = R.costs_fp64(d["masks_n"], d["masks_0"], d["class_n"], d["class_0"])
    d["D2"] = R.costs_fp64(d["masks_m"], d["masks_0"], d["class_m"], d["class_0"])
    return d


def as_kind(masks, kind):
    m = torch.from_numpy(masks)
    if kind == "bool":
        return m.to(DEV)
    if kind == "uint8":
        return (m.to(torch.uint8) * 7).to(DEV)  # non-zero = set
    return m.float().to(DEV)


def instances(d, kind="bool"):
    return [_Inst(torch.from_numpy(d["class_" + s]).to(DEV), as_kind(d["masks_" + s], kind)) for s in ("n", "m", "0")]


def run(d, kind="bool", **kw):
    from mal_amd.matcher import HungarianMatcher
    m = HungarianMatcher(**kw)
    sn, sm = m(*instances(d, kind))
    assert sn.is_cuda and sm.is_cuda and sn.dtype == torch.int64 and sm.dtype == torch.int64 and sn.is_contiguous()
    C1, C2 = m.last_costs
    return sn.cpu().numpy(), sm.cpu().numpy(), C1.cpu().numpy(), C2.cpu().numpy()


@pytest.mark.parametrize("tag", R.CASES)
def test_fixture_cases(tag):
    d = case(tag)
    out = {kind: run(d, kind) for kind in ("bool", "uint8", "float32")}
    sn, sm, C1, C2 = out["bool"]
    err64 = max([float(np.abs(C.astype(np.float64) - D).max()) for C, D in ((C1, d["D1"]), (C2, d["D2"])) if D.size] or [0.0])
    err32 = max([float(np.abs(C.astype(np.float64) - F.astype(np.float64)).max()) for C, F in ((C1, d["C1"]), (C2, d["C2"]))
                 if F.size] or [0.0])
    print("case %s: count %d, |C - fp64| <= %.3g, |C - reference fp32| <= %.3g" % (tag, len(sn), err64, err32))
    assert len(sn) == len(sm) == len(d["pairs"])  # count
    assert np.array_equal(np.stack([sn, sm], 1).reshape(-1, 2), d["pairs"])  # exact integers, ascending target order
    assert C1.dtype == np.float32 and C1.shape == d["C1"].shape and C2.shape == d["C2"].shape
    assert err64 <= 2.5e-7
    assert err32 <= 3e-7
    for kind in ("uint8", "float32"):  # bit-identical whatever the element type of the masks
        for mine, other in zip(out["bool"], out[kind]):
            assert mine.tobytes() == other.tobytes(), kind


def test_weights_scale_the_two_terms():
    d = case("b")
    _, _, C1, C2 = run(d, cost_class=2.0, cost_mask=0.0, cost_dice=0.5)
    D1 = R.costs_fp64(d["masks_n"], d["masks_0"], d["class_n"], d["class_0"], 2.0, 0.5)
    D2 = R.costs_fp64(d["masks_m"], d["masks_0"], d["class_m"], d["class_0"], 2.0, 0.5)
    # costs in [0, 2.5): fp32 spacing <= 2.4e-7 there as well
    assert np.abs(C1 - D1).max() <= 2.5e-7 and np.abs(C2 - D2).max() <= 2.5e-7


@pytest.mark.parametrize("sizes", [(3, 3, 3), (4, 3, 3), (70, 5, 5)], ids=lambda s: "x".join(map(str, s)))
def test_exact_ties(sizes):
    """every mask equal, every class equal: all assignments are optimal; which one is returned is not asserted"""
    H, W = 24, 40
    one = R.ellipse_masks([[12, 20, 5, 9]], H, W)
    d = {"H": H, "W": W}
    for s, n in zip(("n", "m", "0"), sizes):
        d["masks_" + s], d["class_" + s] = np.repeat(one, n, 0), np.zeros(n, dtype=np.int64)
    sn, sm, C1, C2 = run(d)
    count = min(sizes)
    assert len(sn) == len(sm) == count == sizes[2]  # every target is matched on both sides: pair k belongs to target k
    assert len(set(sn.tolist())) == count and len(set(sm.tolist())) == count
    assert sn.min() >= 0 and sn.max() < sizes[0] and sm.min() >= 0 and sm.max() < sizes[1]
    for rows, a in ((sn, "n"), (sm, "m")):
        D = R.costs_fp64(d["masks_" + a], d["masks_0"], d["class_" + a], d["class_0"])
        best = R.assignment_cost(D, *R.linear_sum_assignment(D))
        assert abs(R.assignment_cost(D, rows, np.arange(count)) - best) <= 1e-12


def test_a_non_binary_float_mask_is_refused():
    from mal_amd import _lib
    from mal_amd.matcher import HungarianMatcher
    d = case("b")
    n, m, t = instances(d, "float32")
    m.pred_masks[2, 7, 11] = 0.5
    matcher = HungarianMatcher()
    with pytest.raises(_lib.MalError, match="maskformer_model.py:371"):
        matcher(n, m, t)
    assert matcher.last_costs is None
    m.pred_masks[2, 7, 11] = 1.0
    assert len(matcher(n, m, t)[0]) == len(d["pairs"])  # the flag is per call


def test_determinism():
    d = case("e")
    a, b = run(d), run(d)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_image_synthesis_end_to_end(monkeypatch):
    """dyn_utils.image_synthesis at B=2, 32x64 with a segmenter stand-in that returns case c's permuted masks: the device
    matcher's index tensors go to the kernels as they are (the five-field items), and everything the producer returns is
    bit-equal to a run with a host matcher that returns the fixture's pairs."""
    from mal_amd import dyn_utils
    from mal_amd.matcher import HungarianMatcher
    d = case("c")
    B, H, W = 2, d["H"], d["W"]
    g = torch.Generator().manual_seed(5)
    # sample 1 sees the instances of the two frames in another order
    perm = {0: (np.arange(70), np.arange(66)), 1: (np.random.default_rng(1).permutation(70), np.random.default_rng(2).permutation(66))}
    inv = {b: (np.argsort(p[0]), np.argsort(p[1])) for b, p in perm.items()}
    want = {b: np.stack([inv[b][0][d["pairs"][:, 0]], inv[b][1][d["pairs"][:, 1]]], 1) for b in range(B)}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    frames = {b: (_Inst(dev(d["class_n"][perm[b][0]]), dev(d["masks_n"][perm[b][0]])),
                  _Inst(dev(d["class_m"][perm[b][1]]), dev(d["masks_m"][perm[b][1]]))) for b in range(B)}
    target = _Inst(dev(d["class_0"]), dev(d["masks_0"]))
    color = {f: torch.rand(B, 3, H, W, generator=g).to(DEV) for f in (-1, 0, 1)}
    wl, wn = torch.rand(B, 3, H, W, generator=g).to(DEV), torch.rand(B, 3, H, W, generator=g).to(DEV)

    def produce(matcher_of):
        state = {"b": 0}

        def ins_model(images):
            if state.get("targets_done") is None:  # the first call: the target frames of the whole batch
                state["targets_done"] = True
                return [{"instances": target} for _ in range(B)]
            b = state["b"]
            return [{"instances": frames[b][0]}, {"instances": frames[b][1]}]

        def matcher(ins_last, ins_next, cur):
            out = matcher_of(state["b"])(ins_last, ins_next, cur)
            state["b"] += 1
            return out

        recorded = []
        orig = dyn_utils.BatchSynthesisFn.apply

        def recording(color_last, color_next, items, *rest):
            recorded.append(items)
            return orig(color_last, color_next, items, *rest)

        monkeypatch.setattr(dyn_utils.BatchSynthesisFn, "apply", recording)
        leaves = {f: color[f].clone().requires_grad_(True) for f in (-1, 1)}
        outputs = {("color", -1, 0): leaves[-1], ("color", 1, 0): leaves[1]}
        try:
            assert dyn_utils.image_synthesis({("color", 0, 0): color[0]}, outputs, 0, 0.5, ins_model, matcher) is True
        finally:
            monkeypatch.setattr(dyn_utils.BatchSynthesisFn, "apply", orig)
        ((outputs[("syn", -1, 0)] * wl).sum() + (outputs[("syn", 1, 0)] * wn).sum()).backward()
        (items,) = recorded
        return outputs, leaves, items

    returned = []

    def device_matcher(b):
        m = HungarianMatcher()

        def call(*args):
            returned.append(m(*args))
            return returned[-1]
        return call

    host_matcher = lambda b: (lambda *args: (dev(want[b][:, 0]), dev(want[b][:, 1])))
    out_d, leaves_d, items = produce(device_matcher)
    out_h, leaves_h, _ = produce(host_matcher)
    assert len(items) == B and len(returned) == B
    for b, (item, (sn, sm)) in enumerate(zip(items, returned)):
        assert len(item) == 5 and item[0] == b
        assert item[3] is sn and item[4] is sm and sn.dtype == torch.int64 and sn.is_cuda  # handed over as they are
        assert np.array_equal(torch.stack([sn, sm], 1).cpu().numpy(), want[b])
    for key in (("syn", -1, 0), ("syn", 1, 0), ("syn_region", 0)):
        assert torch.equal(out_d[key], out_h[key]), key
    assert bool((out_d[("syn", -1, 0)] != color[-1]).any())  # the instances moved something
    for f in (-1, 1):
        assert torch.equal(leaves_d[f].grad, leaves_h[f].grad)
