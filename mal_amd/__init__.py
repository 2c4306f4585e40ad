"""mal_amd: MI355X-native photometric reprojection + motion-aware loss path of MAL.

Host side: Python on PyTorch-ROCm mirroring the reference's ``manydepth.layers`` /
``manydepth.loss_utils`` / Trainer warp-loss API.  Device side: hand-written HIP kernels
for gfx950 behind the C ABI of ``include/mal_hip.h`` (``mal_amd/lib/libmal_hip.so``).
There is no CPU implementation in this package: without the HIP library and a GPU the
operators raise.
"""
__version__ = "0.1.0"

__all__ = ["HungarianMatcher", "InstanceSegmenter", "Instances", "instance_inference", "MSDeformAttn", "ms_deform_attn",
           "DynamicDepthEvaluator", "DynamicDepthValPath"]


def __getattr__(name):
    # the temporal-hint producer's matcher (mal_amd/matcher.py); resolved on first use so that `import mal_amd` (and with it
    # `python -m mal_amd.build`) stays free of torch
    if name == "HungarianMatcher":
        from .matcher import HungarianMatcher
        return HungarianMatcher
    # the segmenter's inference tail (mal_amd/instances.py), resolved the same way
    if name in ("InstanceSegmenter", "Instances", "instance_inference"):
        from . import instances
        return getattr(instances, name)
    # the segmenter's multi-scale deformable attention (mal_amd/msda.py), the same way
    if name in ("MSDeformAttn", "ms_deform_attn"):
        from . import msda
        return getattr(msda, name)
    # DynamicDepth's validation metrics (mal_amd/dyn_eval.py), the same way
    if name in ("DynamicDepthEvaluator", "DynamicDepthValPath"):
        from . import dyn_eval
        return getattr(dyn_eval, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
