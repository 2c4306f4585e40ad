"""Golden vectors for the segmenter's inference tail (mal_amd/instances.py) from the REFERENCE's own
``MaskFormer.instance_inference``.

TEST INFRASTRUCTURE ONLY.  Run in the authoring container only (needs the reference checkout):

    python scripts/gen_golden_instances.py /path/to/reference

``mask2former/maskformer_model.py`` is loaded BY FILE PATH with inert stand-ins for the ``detectron2.*`` modules it imports
and for its two relative imports (``.modeling.criterion``, ``.modeling.matcher``); ``Instances`` and ``Boxes`` are two
small classes here (the method of scripts/gen_golden_matcher.py).  ``MaskFormer.instance_inference`` is then called UNBOUND
on a namespace that holds what it reads: ``sem_seg_head.num_classes``, ``num_queries``, ``test_topk_per_image``,
``panoptic_on``, ``metadata`` and ``device``.  Its ``mask_pred`` argument is made by the literal ``F.interpolate`` call of
:222-227 (padded size = 4 (h, w)) followed by the crop to (H, W).  detectron2's ``sem_seg_postprocess`` (:240) is absent
here; at output size = image size it reduces to exactly that crop (its own interpolate is then the identity).  A
``TorchFunctionMode`` records, while the reference runs, what its ``topk`` returned and the quotient of :377, so the class
and mask scores stored here are the reference's own intermediate values, not a re-computation.

Mask logits are multiples of 1/256 within +-16: the x4 weights are dyadic, the upsampled values are exact in fp32
whatever the order of the operations, and the generator asserts that torch's fp32 planes equal the fp64 ones bit for bit.
Mask bytes of a correct implementation are therefore EQUAL to the reference's.

A fixture is written only if (tests/instances_restated.checker, fp64) the T-th and (T+1)-th class scores differ by
>= 1e-5 relative, no two selected scores are closer than that, and no final score lies within 1e-4 of 0.9
(``ins_threshold``); seeds are tried until this holds.  tests/golden/instances_<tag>.npz, a few KB each, data only: the
inputs (mask logits as int16 in units of 1/256), the reference's masks (np.packbits), scores, classes and selected flat
indices in ITS order, the fp64 cls_score / mask_score / score of the checker in the DEFINED order, the reference's own fp32
relative distance from those, and the margins.  Case e also holds ``alt_thing``, a thing table under which the reference
keeps nothing (``alt_count`` = 0).
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch.overrides import TorchFunctionMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import instances_restated as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MARGIN, THRESHOLD, THRESHOLD_MARGIN = 1e-5, 0.9, 1e-4


class Instances:
    def __init__(self, image_size):
        self.image_size = tuple(image_size)


class Boxes:
    def __init__(self, tensor):
        self.tensor = tensor


def import_maskformer(ref):
    def module(name, **names):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in names.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    identity = lambda f: f
    registry = types.SimpleNamespace(register=lambda: identity)
    module("detectron2")
    module("detectron2.config", configurable=identity)
    module("detectron2.data", MetadataCatalog=object)
    module("detectron2.modeling", META_ARCH_REGISTRY=registry, build_backbone=None, build_sem_seg_head=None)
    module("detectron2.modeling.backbone", Backbone=object)
    module("detectron2.modeling.postprocessing", sem_seg_postprocess=None)
    module("detectron2.structures", Boxes=Boxes, ImageList=object, Instances=Instances, BitMasks=object)
    module("detectron2.utils")
    module("detectron2.utils.memory", retry_if_cuda_oom=identity)
    module("m2f_standin")
    module("m2f_standin.modeling")
    module("m2f_standin.modeling.criterion", SetCriterion=object)
    module("m2f_standin.modeling.matcher", HungarianMatcher=object)
    spec = importlib.util.spec_from_file_location("m2f_standin.maskformer_model",
                                                  os.path.join(ref, "mask2former", "maskformer_model.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


class Recorder(TorchFunctionMode):
    """what topk returned, and the last true division of two tensors (:377)"""

    def __init__(self):
        super().__init__()
        self.topk, self.quotient = None, None

    def __torch_function__(self, func, types_, args=(), kwargs=None):
        kwargs = kwargs or {}
        out = func(*args, **kwargs)
        name = getattr(func, "__name__", "")
        if name == "topk":
            self.topk = (out[0].clone(), out[1].clone())
        elif name in ("__truediv__", "true_divide", "div") and "rounding_mode" not in kwargs and torch.is_tensor(out) \
                and out.is_floating_point() and out.dim() == 1:
            self.quotient = out.clone()
        return out


def run_reference(M, logits, planes, H, W, T, thing):
    """-> the reference's result for one image + its own intermediates"""
    Q, K = logits.shape[0], logits.shape[1] - 1
    h, w = planes.shape[-2:]
    things = {} if thing is None else {100 + c: c for c in range(K) if thing[c]}
    ns = types.SimpleNamespace(sem_seg_head=types.SimpleNamespace(num_classes=K), num_queries=Q, test_topk_per_image=T,
                               panoptic_on=thing is not None, device=torch.device("cpu"),
                               metadata=types.SimpleNamespace(thing_dataset_id_to_contiguous_id=things))
    mask_pred_results = torch.from_numpy(planes)[None]
    mask_pred_results = F.interpolate(  # maskformer_model.py:222-227, images.tensor.shape[-2:] = 4 (h, w)
        mask_pred_results,
        size=(4 * h, 4 * w),
        mode="bilinear",
        align_corners=False,
    )
    exact = R.upsample_x4(planes, 4 * h, 4 * w)
    assert np.array_equal(mask_pred_results[0].numpy().astype(np.float64), exact), "the fp32 upsample is not exact"
    mask_pred = mask_pred_results[0][:, :H, :W]  # sem_seg_postprocess at output size = image size
    with Recorder() as rec:
        result = M.MaskFormer.instance_inference(ns, torch.from_numpy(logits), mask_pred)
    values, indices = rec.topk
    keep = torch.ones(T, dtype=torch.bool) if thing is None else torch.as_tensor(thing)[indices % K]
    assert result.image_size == (H, W) and len(result.pred_classes) == int(keep.sum())
    assert torch.equal(result.pred_classes, (indices % K)[keep])
    n = int(keep.sum())
    mask_scores = rec.quotient if n else torch.zeros(0)
    assert mask_scores.shape == (n,) and torch.equal(values[keep] * mask_scores, result.scores)
    return {"flat": indices[keep].numpy(), "masks": result.pred_masks.numpy() != 0, "scores": result.scores.numpy(),
            "classes": result.pred_classes.numpy(), "cls_score": values[keep].numpy(), "mask_score": mask_scores.numpy()}


def dyadic(rng, shape, lo=-16.0, hi=16.0):
    return (rng.integers(int(lo * R.MASK_UNIT), int(hi * R.MASK_UNIT) + 1, shape).astype(np.float32) / R.MASK_UNIT)


def make_inputs(tag, rng, Q, K, h, w):
    """logits, planes, thing, alt_thing"""
    logits = (rng.standard_normal((Q, K + 1)) * 2.0).astype(np.float32)
    # smooth-ish planes with both signs: a coarse random field plus noise, in units of 1/256
    planes = dyadic(rng, (Q, h, w), -6.0, 6.0) + dyadic(rng, (Q, 1, 1), -3.0, 3.0)
    planes = np.clip(planes, -16.0, 16.0).astype(np.float32)
    thing = alt = None
    if tag == "d":
        thing = np.zeros(K, dtype=bool)
        thing[rng.permutation(K)[:3]] = True
    if tag == "e":
        # every query peaked on one of the classes 0..5: the six peaks are the top six; query 0 is all-negative; query 1
        # holds exact zeros on a block of texels (v == 0 pixels, which must stay unset) between a positive and a negative part
        peak = rng.permutation(6)
        logits[np.arange(Q), peak] += 8.0
        planes[0] = -np.abs(planes[0]) - 1.0 / R.MASK_UNIT
        planes[1, :, :4] = np.abs(planes[1, :, :4]) + 0.5
        planes[1, :, 4:7] = 0.0
        planes[1, :, 7:] = -np.abs(planes[1, :, 7:]) - 0.5
        alt = np.zeros(K, dtype=bool)
        alt[6:] = True  # no selected class is a thing: nothing survives
    return logits, planes, thing, alt


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    M = import_maskformer(sys.argv[1])
    torch.set_num_threads(1)  # one summation order of the reference's fp32 sums, whatever the host
    for tag, (Q, K, h, w, H, W, T) in R.CASES.items():
        for seed in range(1000):
            rng = np.random.default_rng(1000 * ord(tag) + seed)
            logits, planes, thing, alt = make_inputs(tag, rng, Q, K, h, w)
            c = R.checker(logits, planes, H, W, T, thing)
            near = float(np.abs(c["score"] - THRESHOLD).min()) if len(c["score"]) else np.inf
            if c["margin_cut"] >= MARGIN and c["margin_sel"] >= MARGIN and near >= THRESHOLD_MARGIN:
                break
        else:
            raise SystemExit("case %s: no inputs with the required margins found" % tag)
        ref = run_reference(M, logits, planes, H, W, T, thing)
        # the reference's selection is the checker's, as a set; align the reference's rows with the defined order
        assert sorted(ref["flat"].tolist()) == sorted(c["flat"].tolist()), tag
        at = {f: k for k, f in enumerate(ref["flat"].tolist())}
        rows = np.array([at[f] for f in c["flat"].tolist()], dtype=np.int64)
        assert np.array_equal(ref["masks"][rows], c["masks"]), tag
        assert np.array_equal(ref["classes"][rows], c["classes"]), tag
        dist = np.array([R.rel_dist(ref[k][rows], c[k]) for k in ("cls_score", "mask_score")] +
                        [R.rel_dist(ref["scores"][rows], c["score"])])
        assert np.all(np.isfinite(dist)), (tag, dist)
        extra = {}
        if alt is not None:
            none = run_reference(M, logits, planes, H, W, T, alt)
            assert len(none["flat"]) == 0 and none["masks"].shape == (0, H, W)
            extra = {"alt_thing": alt, "alt_count": np.int64(len(none["flat"]))}
        if tag == "e":  # what the case is for
            k0, k1 = list(c["query"]).index(0), list(c["query"]).index(1)
            v1 = R.upsample_x4(planes[1], H, W)
            assert not c["masks"][k0].any() and c["score"][k0] == 0 and ref["scores"][rows][k0] == 0
            assert (v1 == 0).any() and not c["masks"][k1][v1 == 0].any() and c["masks"][k1].any()
        if tag == "b":
            assert len(set(c["query"].tolist())) < len(c["query"])  # a query fills several slots
        q8 = np.round(planes.astype(np.float64) * R.MASK_UNIT).astype(np.int16)
        assert np.array_equal(q8.astype(np.float32) / R.MASK_UNIT, planes)
        np.savez(os.path.join(OUT, "instances_%s.npz" % tag), dims=np.array([Q, K, h, w, H, W, T], dtype=np.int64),
                 logits=logits, planes_q8=q8, thing=(thing if thing is not None else np.zeros(0, dtype=bool)),
                 ref_masks_bits=np.packbits(ref["masks"].reshape(-1)), ref_scores=ref["scores"], ref_classes=ref["classes"],
                 ref_flat=ref["flat"], cls_score=c["cls_score"], mask_score=c["mask_score"], score=c["score"], ref_dist=dist,
                 margins=np.array([c["margin_cut"], c["margin_sel"], near], dtype=np.float64), **extra)
        print("case %s seed %d: Q=%d K=%d %dx%d -> %dx%d T=%d kept %d, margins %.3g / %.3g / %.3g, reference fp32 distance "
              "cls %.3g mask %.3g score %.3g" % ((tag, seed, Q, K, h, w, H, W, T, len(c["flat"]), c["margin_cut"],
                                                   c["margin_sel"], near) + tuple(dist)))


if __name__ == "__main__":
    main()
