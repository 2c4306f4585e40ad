"""CPU: the checker of the segmenter's inference tail (tests/instances_restated.py) against the reference's own outputs
(tests/golden/instances_*.npz, scripts/gen_golden_instances.py) and against ATen's upsample; the argument validation of
``mal_instances`` (no device is needed: nothing is launched); ``mal_amd.instances.Instances`` and the refusal of CPU
tensors."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import instances_restated as R


@pytest.fixture(scope="module")
def lib():
    from mal_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("tag", list(R.CASES))
def test_checker_reproduces_the_reference(tag):
    d = R.load_case(tag)
    assert (d["Q"], d["K"], d["h"], d["w"], d["H"], d["W"], d["T"]) == R.CASES[tag]
    assert np.array_equal(d["planes"] * R.MASK_UNIT, np.round(d["planes"] * R.MASK_UNIT)) and np.abs(d["planes"]).max() <= 16
    c = R.checker(d["logits"], d["planes"], d["H"], d["W"], d["T"], d["thing"])
    # the fixture's margins: the selection and the 0.9 threshold are not a matter of rounding
    assert d["margins"][0] >= 1e-5 and d["margins"][1] >= 1e-5 and d["margins"][2] >= 1e-4
    assert np.isclose(c["margin_cut"], d["margins"][0], rtol=1e-6) and np.isclose(c["margin_sel"], d["margins"][1], rtol=1e-6)
    # the selected (query, class) set is the reference's
    assert sorted(c["flat"].tolist()) == sorted(d["ref_flat"].tolist())
    assert len(set(c["flat"].tolist())) == len(c["flat"])
    at = {f: k for k, f in enumerate(d["ref_flat"].tolist())}
    rows = np.array([at[f] for f in c["flat"].tolist()], dtype=np.int64)
    assert np.array_equal(d["ref_masks"][rows], c["masks"])  # equal, no exemptions
    assert np.array_equal(d["ref_classes"][rows], c["classes"])
    assert np.array_equal(c["flat"] // d["K"], c["query"]) and np.all(np.diff(c["cls_score"]) < 0)  # the defined order
    # the stored fp64 columns are the checker's (exp of another libm: a few fp64 ulp)
    for k in ("cls_score", "mask_score", "score"):
        assert c[k].shape == d[k].shape and R.rel_dist(c[k], d[k]) <= 1e-12, k
    dist = R.rel_dist(d["ref_scores"][rows], c["score"])
    print("case %s: kept %d, reference fp32 distance of the score %.3g (stored %.3g)" % (tag, len(rows), dist, d["ref_dist"][2]))
    assert dist <= 1.25 * d["ref_dist"][2]
    assert np.all(d["ref_dist"] < 1e-6)


def test_case_e_is_what_it_is_for():
    d = R.load_case("e")
    c = R.checker(d["logits"], d["planes"], d["H"], d["W"], d["T"], None)
    k0, k1 = list(c["query"]).index(0), list(c["query"]).index(1)
    assert not c["masks"][k0].any() and c["mask_score"][k0] == 0 and c["score"][k0] == 0  # the all-negative query
    v1 = R.upsample_x4(d["planes"][1], d["H"], d["W"])
    assert (v1 == 0).sum() > 0 and not c["masks"][k1][v1 == 0].any() and c["masks"][k1].any()  # v == 0 stays unset
    z = np.load(R.GOLDEN + "/instances_e.npz")
    none = R.checker(d["logits"], d["planes"], d["H"], d["W"], d["T"], z["alt_thing"])
    assert int(z["alt_count"]) == 0 and len(none["flat"]) == 0 and none["masks"].shape == (0, d["H"], d["W"])


def test_case_b_repeats_a_query_and_f_fills_the_limit():
    from mal_amd import _lib
    b = R.load_case("b")
    c = R.checker(b["logits"], b["planes"], b["H"], b["W"], b["T"], None)
    assert len(set(c["query"].tolist())) < len(c["query"])
    assert R.CASES["f"][6] == _lib.MATCH_MAX


SHAPES = sorted({(h, w, H, W) for (_, _, h, w, H, W, _) in R.CASES.values()} | {(1, 1, 4, 4), (1, 1, 1, 1), (2, 3, 8, 12),
                                                                               (48, 160, 192, 640)})


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample_rule_is_atens(shape):
    """dyadic inputs: every order of the operations is exact in fp32, so ATen's fp32 result IS the fp64 rule"""
    h, w, H, W = shape
    rng = np.random.default_rng(h * 1000 + w)
    x = rng.integers(-16 * R.MASK_UNIT, 16 * R.MASK_UNIT + 1, (3, h, w)).astype(np.float32) / R.MASK_UNIT
    theirs = F.interpolate(torch.from_numpy(x)[None], size=(4 * h, 4 * w), mode="bilinear", align_corners=False)[0, :, :H, :W]
    mine = R.upsample_x4(x, H, W)
    assert mine.shape == (3, H, W) and np.array_equal(theirs.numpy().astype(np.float64), mine)
    i0, i1, wt = R.taps(4 * w, w)
    assert set(np.unique(wt[2:-2]).tolist()) <= {0.125, 0.375, 0.625, 0.875}
    assert wt[0] == 0 and wt[1] == 0 and i0[-1] == i1[-1] == w - 1 and i0[-2] == i1[-2] == w - 1


def test_torch_tail_agrees_with_the_checker_on_the_cpu():
    d = R.load_case("d")
    out, = R.torch_tail(torch.from_numpy(d["logits"])[None], torch.from_numpy(d["planes"])[None], d["H"], d["W"], d["T"], d["thing"])
    assert sorted(out["flat"].tolist()) == sorted(d["ref_flat"].tolist())
    at = {f: k for k, f in enumerate(out["flat"].tolist())}
    rows = [at[f] for f in d["ref_flat"].tolist()]
    assert np.array_equal(out["masks"].numpy()[rows], d["ref_masks"])
    assert np.array_equal(out["scores"].numpy()[rows], d["ref_scores"])  # the same operators: the same bits


def test_general_seed_on_the_cpu():
    """the general fp32 case of the device test (N(0, 4) logits, Q=100, 48x160 -> 192x640): torch's own fp32 planes have no
    pixel on the wrong side of zero outside the rounding band, and the band holds far fewer than 1e-5 of the pixels"""
    _, planes = R.general_inputs()
    H, W = 192, 640
    up = F.interpolate(torch.from_numpy(planes)[None], size=(H, W), mode="bilinear", align_corners=False)[0]
    outside, differ, inside = R.band_report((up > 0).numpy(), planes, H, W)
    total = planes.shape[0] * H * W
    print("seed %d: %d of %d pixels differ (%d outside the band), %d inside it" % (R.GENERAL_SEED, differ, total, outside, inside))
    assert outside == 0 and differ <= 1e-5 * total and inside <= 1e-5 * total


def test_argument_validation_without_device(lib):
    from mal_amd import _lib
    ok = dict(N=1, Q=10, K=8, h=6, w=10, H=24, W=40, topk=10)
    size = lambda **kw: lib.mal_instances_workspace_bytes(*[{**ok, **kw}[k] for k in ("N", "Q", "K", "h", "w", "H", "W", "topk")])
    buf = (ctypes.c_uint8 * 64)()
    addr = ctypes.addressof(buf)

    def call(null=(), **kw):
        a = _lib.InstancesArgs()
        for name in ("pred_logits", "pred_masks", "count", "masks", "scores", "classes", "query", "cls_score", "mask_score", "ws"):
            setattr(a, name, None if name in null else addr)  # never dereferenced: every call below is refused
        for k, v in {**ok, **kw}.items():
            setattr(a, k, v)
        a.ws_bytes = 0 if "ws_bytes" in null else 1 << 40
        return lib.mal_instances(ctypes.byref(a))

    assert size() > 0
    assert lib.mal_instances(None) == -1
    for name in ("pred_logits", "pred_masks", "count", "masks", "scores", "classes", "query", "cls_score", "mask_score", "ws"):
        assert call(null=(name,)) == -1, name
    bad = [dict(topk=81), dict(Q=1, K=8, topk=9), dict(Q=100, topk=129), dict(topk=0), dict(H=20), dict(H=25), dict(W=36),
           dict(W=41), dict(H=0), dict(N=0), dict(Q=0), dict(K=0), dict(h=0), dict(Q=2049, K=8), dict(Q=200, K=82)]
    for kw in bad:
        assert size(**kw) == 0, kw
        assert call(**kw) == -1, kw
    for kw in (dict(H=21), dict(W=37), dict(Q=200, K=80, topk=128), dict(Q=100, topk=128)):
        assert size(**kw) > 0, kw
    assert call(null=("ws_bytes",)) == -3  # a workspace that is too small: MAL_EWORKSPACE, still nothing launched
    assert size(N=2) > size(N=1)


def test_instances_indexing_and_len():
    from mal_amd import _lib
    from mal_amd.instances import Instances
    masks = (torch.arange(5 * 2 * 3).view(5, 2, 3) % 2).to(torch.uint8)
    inst = Instances((2, 3), masks, torch.tensor([0.95, 0.5, 0.99, 0.1, 0.91]), torch.arange(5), query=torch.arange(5) * 2)
    assert len(inst) == 5 and inst.image_size == (2, 3)
    sel = inst[inst.scores > 0.9]
    assert len(sel) == 3 and sel.pred_classes.tolist() == [0, 2, 4] and torch.equal(sel.pred_masks, masks[[0, 2, 4]])
    assert sel.query.tolist() == [0, 4, 8] and sel.image_size == (2, 3)
    assert inst[torch.tensor([3, 1])].pred_classes.tolist() == [3, 1]
    assert inst[1:3].pred_classes.tolist() == [1, 2] and len(inst[5:]) == 0 and inst[5:].pred_masks.shape == (0, 2, 3)
    assert len(inst[2]) == 1 and inst[2].pred_classes.tolist() == [2] and inst[-1].pred_classes.tolist() == [4]
    with pytest.raises(IndexError):
        inst[5]
    with pytest.raises(AttributeError):
        inst.pred_boxes
    with pytest.raises(_lib.MalError):
        Instances((2, 3), masks, torch.zeros(4), torch.arange(5))
    import mal_amd
    assert mal_amd.Instances is Instances and mal_amd.InstanceSegmenter is mal_amd.instances.InstanceSegmenter


def test_cpu_tensors_are_refused(lib):
    from mal_amd import _lib
    from mal_amd.instances import InstanceSegmenter, instance_inference
    seg = InstanceSegmenter(lambda x: {}, [103.5, 116.3, 123.7], [57.4, 57.1, 58.4])
    with pytest.raises(_lib.MalError, match="device tensor"):
        seg(torch.rand(2, 3, 24, 40))
    with pytest.raises(_lib.MalError, match="device tensor"):
        instance_inference(torch.zeros(1, 10, 9), torch.zeros(1, 10, 6, 10), (24, 40), topk=10)
    # the input convention: BGR x 255, normalised, zero-padded at the right and bottom to a multiple of 32
    x = torch.rand(2, 3, 24, 40)
    y = seg.preprocess(x)
    assert y.shape == (2, 3, 32, 64) and bool((y[:, :, 24:] == 0).all()) and bool((y[:, :, :, 40:] == 0).all())
    want = (x[:, [2, 1, 0]] * 255 - torch.tensor([103.5, 116.3, 123.7]).view(1, 3, 1, 1)) / torch.tensor([57.4, 57.1, 58.4]).view(1, 3, 1, 1)
    assert torch.equal(y[:, :, :24, :40], want)
    assert seg.preprocess(torch.rand(1, 3, 192, 640)).shape == (1, 3, 192, 640)
