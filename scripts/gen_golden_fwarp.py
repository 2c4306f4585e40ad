"""Golden vectors for mal_amd.rigid_warp from the REFERENCE's own ``forward_warp`` (dynamicdepth/rigid_warp.py:534-597).

TEST INFRASTRUCTURE ONLY.  Run in the authoring container only (needs the reference checkout), after
scripts/gen_golden_msda.py:

    python scripts/gen_golden_fwarp.py /path/to/reference

``dynamicdepth/rigid_warp.py`` is loaded BY FILE PATH.  It imports ``coalesce`` from ``torch_sparse`` (:7), a package of
compiled CUDA kernels that is not installed.  The stand-in used here is NOT INERT: its ``coalesce(index, value, m, n,
op='max')`` does what the package documents -- row-major sorted unique indices, duplicates reduced by max -- and the
reference's z-buffer is whatever it returns.  So these fixtures are "the reference's program text on the documented
behaviour of its dependency", not a run of the dependency's kernels.  ``matplotlib`` and ``pdb`` are imported by the file
and never used by ``forward_warp``; matplotlib gets an empty stand-in.

The module caches its pixel grid in a global, ``pixel_coords``; its cache test compares heights only and the grid keeps the
dtype of the first call, so the global is reset before every case.  For the same reason, and because
``sparse.FloatTensor`` is fp32 only, the reference runs in fp32 only; the fp64 side of every gate is
tests/fwarp_restated.py, which this script holds to the reference's fp32 outputs BIT FOR BIT on every case.

tests/golden/fwarp_<case>.npz, data only, for the 20 cases of fwarp_restated.GOLDEN_CASES: the inputs (img, depth, pose, K,
up) and the reference's three outputs (img_w, depth_w, valid).
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
from tests import fwarp_restated as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def coalesce(index, value, m, n, op="add"):
    """torch_sparse.coalesce as documented: (2,E) indices into an m x n matrix -> row-major sorted unique indices, the
    values of duplicates reduced by ``op``"""
    assert op == "max" and index.shape[0] == 2 and value.dim() == 1
    key = index[0] * n + index[1]
    uniq, inverse = torch.unique(key, sorted=True, return_inverse=True)
    out = torch.full((uniq.numel(),), -float("inf"), dtype=value.dtype).scatter_reduce(0, inverse, value, "amax")
    return torch.stack([torch.div(uniq, n, rounding_mode="floor"), uniq % n]), out


def import_reference(ref):
    sparse = types.ModuleType("torch_sparse")
    sparse.coalesce = coalesce
    stand_ins = {"torch_sparse": sparse}
    try:
        import matplotlib.pyplot  # noqa: F401
    except Exception:
        mpl = types.ModuleType("matplotlib")
        mpl.pyplot = types.ModuleType("matplotlib.pyplot")
        stand_ins.update({"matplotlib": mpl, "matplotlib.pyplot": mpl.pyplot})
    sys.modules.update(stand_ins)
    spec = importlib.util.spec_from_file_location("fwarp_reference", os.path.join(ref, "dynamicdepth", "rigid_warp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for k in stand_ins:
        del sys.modules[k]
    return mod


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = import_reference(sys.argv[1])
    torch.set_num_threads(1)
    for name in R.GOLDEN_CASES:
        c = R.make_case(name)
        ref.pixel_coords = None
        with torch.no_grad():
            img_w, depth_w, valid = ref.forward_warp(c["img"], c["depth"], c["pose"], c["K"], upscale=c["up"],
                                                     rotation_mode="euler", padding_mode="zeros")
        mine = R.forward_warp(c["img"], c["depth"], c["pose"], c["K"], c["up"], torch.float32)
        for k, t in (("img_w", img_w), ("depth_w", depth_w), ("valid", valid)):
            assert t.dtype == torch.float32 and t.shape == mine[k].shape, (name, k, t.shape, mine[k].shape)
            assert np.array_equal(t.numpy().view(np.int32), mine[k].numpy().view(np.int32)), \
                "%s: the restatement's %s is not the reference's bit for bit" % (name, k)
        np.savez_compressed(os.path.join(OUT, "fwarp_%s.npz" % name), img=c["img"].numpy(), depth=c["depth"].numpy(),
                            pose=c["pose"].numpy(), K=c["K"].numpy(), up=np.int64(c["up"]), img_w=img_w.numpy(),
                            depth_w=depth_w.numpy(), valid=valid.numpy())
        print("case %s: %s, %.0f %% holes, %.0f %% valid" % (name, tuple(img_w.shape), 100 * float((mine["fw_val"] == 0).float().mean()),
                                                            100 * float(valid.mean())))


if __name__ == "__main__":
    main()
