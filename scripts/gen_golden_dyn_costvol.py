"""Golden vectors for mal_amd.costvol's occlusion-aware cost volume from the REFERENCE's own
``ResnetEncoderMatching.match_features`` (dynamicdepth/networks/resnet_encoder.py:148-249).

TEST INFRASTRUCTURE ONLY.  Run in the authoring container only (needs the reference checkout):

    python scripts/gen_golden_dyn_costvol.py /path/to/reference

``dynamicdepth/networks/resnet_encoder.py`` is loaded BY FILE PATH with an inert stand-in for torchvision (its ResNet classes
are only subclassed, and instantiated by constructors that are not called here) and ``dynamicdepth.layers`` loaded by path as
well.  ``match_features`` is called unbound on a namespace object that carries what it reads from ``self``: the reference's own
``BackprojectDepth`` / ``Project3D`` objects, the warp depths, the matching size.  Upstream hard-codes ``repeat([96,64,1,1])``
(:194), so every case has D = 96, C = 64.

tests/golden/dyn_costvol_<case>.npz, data only, for the ten cases of dyn_costvol_restated.GOLDEN_CASES: the inputs (features
as fp16, they are fp16-representable), the options and the reference's two outputs.  tests/dyn_costvol_restated.py is held to
them BIT FOR BIT here.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dyn_costvol_restated as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def import_reference(ref):
    tv, models = types.ModuleType("torchvision"), types.ModuleType("torchvision.models")
    models.ResNet = type("ResNet", (torch.nn.Module,), {})
    models.resnet = types.ModuleType("torchvision.models.resnet")
    tv.models = models
    pkg = types.ModuleType("dynamicdepth")
    pkg.__path__ = [os.path.join(ref, "dynamicdepth")]
    stand_ins = {"torchvision": tv, "torchvision.models": models, "torchvision.models.resnet": models.resnet, "dynamicdepth": pkg}
    saved = {k: sys.modules.get(k) for k in stand_ins}
    sys.modules.update(stand_ins)
    layers = _load("dynamicdepth.layers", os.path.join(ref, "dynamicdepth", "layers.py"))
    enc = _load("dyn_costvol_reference", os.path.join(ref, "dynamicdepth", "networks", "resnet_encoder.py"))
    for k, v in saved.items():
        if v is None:
            del sys.modules[k]
        else:
            sys.modules[k] = v
    return layers, enc.ResnetEncoderMatching


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    layers, Enc = import_reference(sys.argv[1])
    torch.set_num_threads(1)
    for name in R.GOLDEN_CASES:
        c = R.golden_case(name)
        B, C, h, w = c["cur"].shape
        D = c["bins"].numel()
        me = types.SimpleNamespace(num_depth_bins=D, matching_height=h, matching_width=w, set_missing_to_max=True,
                                   warp_depths=c["bins"].view(D, 1, 1, 1).expand(D, 1, h, w).contiguous().float(),
                                   backprojector=layers.BackprojectDepth(batch_size=D, height=h, width=w),
                                   projector=layers.Project3D(batch_size=D, height=h, width=w))
        with torch.no_grad():
            cv, miss = Enc.match_features(me, c["cur"], c["look"], c["poses"], c["K"], c["invK"], c["images"], c["cv_min"], c["aug"],
                                          c["set_1"], c["pool"], c["pool_r"], c["pool_th"])
            mine = R.run_case(c, torch.float32)
        for k, a, b in (("cost_volume", cv, mine[0]), ("missing", miss, mine[1])):
            assert a.dtype == torch.float32 and a.shape == b.shape, (name, k, a.shape, b.shape)
            assert np.array_equal(a.numpy().view(np.int32), b.numpy().view(np.int32)), \
                "%s: the restatement's %s is not the reference's bit for bit" % (name, k)
        assert all(torch.equal(c[k], c[k].half().float()) for k in ("cur", "look", "images"))
        np.savez_compressed(os.path.join(OUT, "dyn_costvol_%s.npz" % name), cur=c["cur"].half().numpy(), look=c["look"].half().numpy(),
                            poses=c["poses"].numpy(), K=c["K"].numpy(), invK=c["invK"].numpy(), images=c["images"].half().numpy(),
                            bins=c["bins"].numpy(), aug=c["aug"].numpy(), cv_min=np.bool_(c["cv_min"]), set_1=np.bool_(c["set_1"]),
                            pool=np.bool_(c["pool"]), pool_r=np.int64(c["pool_r"]), pool_th=np.float64(c["pool_th"]),
                            cost_volume=cv.numpy(), missing=miss.numpy())
        print("case %s: %s, %.1f %% missing" % (name, tuple(cv.shape), 100 * float(miss.mean())))


if __name__ == "__main__":
    main()
