"""Golden vectors for mal_amd.msda from the REFERENCE's own ``ms_deform_attn_core_pytorch`` and ``MSDeformAttn``.

TEST INFRASTRUCTURE ONLY.  Run in the authoring container only (needs the reference checkout):

    python scripts/gen_golden_msda.py /path/to/reference

``ops/functions/ms_deform_attn_func.py`` and ``ops/modules/ms_deform_attn.py`` are loaded BY FILE PATH under a stand-in
package, with an inert, empty module in place of the CUDA extension ``MultiScaleDeformableAttention``.  With it the
module's ``try`` around ``MSDeformAttnFunction.apply`` fails and its ``except`` branch calls
``ms_deform_attn_core_pytorch``, so the module's own ``forward`` runs on the CPU, in fp32 and (``.double()``) in fp64.

tests/golden/msda_<tag>.npz, data only.  Operator cases (tests/msda_restated.CASES): the inputs as integers (value in
units of 1/16, locations and weights in units of 1/4096: every one an fp32 number, so fp32 and fp64 see the same
inputs), ``ref64`` the reference's fp64 output, ``ref32_ulps`` its fp32 output as the integer distance of its bit
pattern from the rounded fp64 output, ``ref_dist`` = ||ref32 - ref64|| / ||ref64||.  Case x is exact: locations are
multiples of 1/128, weights multiples of 1/64 that sum to 1, values integers in [-8, 8]; every product and partial sum
is exact in fp32 and the generator asserts ref32 == ref64 bit for bit.  Module cases m2 / m4: the state dict (random,
non-zero in all four layers), the inputs, the module's fp32 and fp64 outputs, its fp32 offsets and logits, and the
state dict's keys and shapes as the reference's module reports them.
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
from tests import msda_restated as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def import_reference(ref):
    ops = os.path.join(ref, "mask2former", "modeling", "pixel_decoder", "ops")
    sys.modules["MultiScaleDeformableAttention"] = types.ModuleType("MultiScaleDeformableAttention")  # inert

    def package(name):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
        return m

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    package("msda_standin")
    functions = package("msda_standin.functions")
    package("msda_standin.modules")
    func = load("msda_standin.functions.ms_deform_attn_func", os.path.join(ops, "functions", "ms_deform_attn_func.py"))
    functions.MSDeformAttnFunction = func.MSDeformAttnFunction
    mod = load("msda_standin.modules.ms_deform_attn", os.path.join(ops, "modules", "ms_deform_attn.py"))
    del sys.modules["MultiScaleDeformableAttention"]
    return func, mod


def quantised(a, unit, dtype):
    q = np.round(np.asarray(a, np.float64) * unit).astype(dtype)
    back = q.astype(np.float32) / np.float32(unit)
    assert np.array_equal(back.astype(np.float64) * unit, q.astype(np.float64))
    return q, back


def operator_inputs(tag, rng):
    N, M, D, P, levels, Lq = R.CASES[tag]
    L = len(levels)
    start, S = R.starts_of(levels)
    Lq = S if Lq is None else Lq
    if tag == "x":
        value = rng.integers(-8, 9, (N, S, M, D)).astype(np.float64)
        loc = rng.integers(-32, 161, (N, Lq, M, L, P, 2)) / 128.0
        weights = rng.multinomial(64, np.full(L * P, 1.0 / (L * P)), (N, Lq, M)).reshape(N, Lq, M, L, P) / 64.0
    else:
        value = np.clip(rng.standard_normal((N, S, M, D)) * 2.0, -7.9, 7.9)
        spread = {"a": 0.1, "b": 0.6, "c": 0.25, "d": 0.3}[tag]
        loc = rng.random((N, Lq, 1, L, 1, 2)) + spread * rng.standard_normal((N, Lq, M, L, P, 2))
        loc = np.clip(loc, -0.49, 1.49)
        weights = R.softmax(rng.standard_normal((N, Lq, M, L * P)) * 1.5).reshape(N, Lq, M, L, P)
    vq, value = quantised(value, R.VALUE_UNIT, np.int16)
    lq, loc = quantised(loc, R.LOC_UNIT, np.int16)
    wq, weights = quantised(weights, R.WEIGHT_UNIT, np.uint16)
    if tag == "b":  # samples at x*W - 0.5 in {-1, 0, W-1, W} and the same in y, as fp32 numbers (not on the 1/4096 grid)
        H, W = levels[0]
        loc = loc.copy()
        xs = (np.array([-1, 0, W - 1, W]) + 0.5) / W
        ys = (np.array([-1, 0, H - 1, H]) + 0.5) / H
        k = 0
        for xv in xs:
            for yv in ys:
                loc[0, k % Lq, k % M, 0, (k // M) % P] = (xv, yv)
                k += 1
        loc = loc.astype(np.float32)
        lq = None
    return value, levels, start, loc, weights, (vq, lq, wq)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    func, modfile = import_reference(sys.argv[1])
    torch.set_num_threads(1)
    T = torch.from_numpy
    for tag in R.CASES:
        rng = np.random.default_rng(7000 + ord(tag))
        value, levels, start, loc, weights, (vq, lq, wq) = operator_inputs(tag, rng)
        shp = torch.tensor(levels, dtype=torch.int64)
        ref32 = func.ms_deform_attn_core_pytorch(T(value), shp, T(loc), T(weights)).numpy()
        ref64 = func.ms_deform_attn_core_pytorch(T(value).double(), shp, T(loc).double(), T(weights).double()).numpy()
        assert ref32.dtype == np.float32 and ref64.dtype == np.float64
        chk = R.core(value, levels, start, loc, weights, np.float64)
        assert R.rel_dist(chk, ref64) <= 1e-12, (tag, R.rel_dist(chk, ref64))
        dist = R.rel_dist(ref32, ref64)
        outside = float(np.mean((loc < 0) | (loc > 1)))
        if tag == "x":
            assert np.array_equal(ref32.view(np.int32), ref64.astype(np.float32).view(np.int32)), "case x is not exact"
            assert np.array_equal(ref64.astype(np.float32).astype(np.float64), ref64)
            assert np.array_equal(R.core(value, levels, start, loc, weights, np.float32).view(np.int32), ref32.view(np.int32))
        ulps = ref32.view(np.int32) - ref64.astype(np.float32).view(np.int32)  # (wraps, and is undone the same way)
        extra = {"loc_q": lq} if lq is not None else {"loc": loc}
        np.savez_compressed(os.path.join(OUT, "msda_%s.npz" % tag), shapes=np.array(levels, np.int64),
                            start=np.array(start, np.int64), value_q=vq, weights_q=wq, ref64=ref64, ref32_ulps=ulps,
                            ref_dist=np.float64(dist), **extra)
        print("case %s: out %s, %.0f %% of the coordinates outside [0,1], reference fp32 distance %.3g, largest ulp offset %d"
              % (tag, ref32.shape, 100 * outside, dist, np.abs(ulps).max()))
    cfg = R.MODULE_CFG
    for tag, ref_dim in R.MODULE_CASES.items():
        rng = np.random.default_rng(7100 + ref_dim)
        torch.manual_seed(7100 + ref_dim)
        m = modfile.MSDeformAttn(**cfg)
        C = cfg["d_model"]
        with torch.no_grad():
            for name, prm in m.named_parameters():
                prm.copy_(T(rng.standard_normal(tuple(prm.shape)).astype(np.float32)) * (0.5 if name.endswith("bias") else C ** -0.5))
        start, S = R.starts_of(R.MODULE_LEVELS)
        N, Lq, L = R.MODULE_N, R.MODULE_LQ, cfg["n_levels"]
        query = rng.standard_normal((N, Lq, C)).astype(np.float32)
        inp = rng.standard_normal((N, S, C)).astype(np.float32)
        ref = rng.random((N, Lq, L, ref_dim)).astype(np.float32)
        if ref_dim == 4:
            ref[..., 2:] = 0.1 + 0.4 * ref[..., 2:]
        mask = None
        if tag == "m2":
            mask = rng.random((N, S)) < 0.2
            assert mask.any() and not mask.all()
        shp, sti = torch.tensor(R.MODULE_LEVELS, dtype=torch.int64), torch.tensor(start, dtype=torch.int64)
        tm = None if mask is None else T(mask)
        with torch.no_grad():
            out32 = m(T(query), T(ref), T(inp), shp, sti, tm).numpy()
            offsets = m.sampling_offsets(T(query)).numpy()
            logits = m.attention_weights(T(query)).numpy()
            sd = {k: v.numpy().copy() for k, v in m.state_dict().items()}
            out64 = m.double()(T(query).double(), T(ref).double(), T(inp).double(), shp, sti, tm).numpy()
        assert tuple(sd) == R.STATE_KEYS and all(np.abs(v).min() > 0 for v in sd.values())
        chk, _, _ = R.module_forward(sd, query, ref, inp, R.MODULE_LEVELS, start, mask, np.float64)
        assert R.rel_dist(chk, out64) <= 1e-12, (tag, R.rel_dist(chk, out64))
        dist = R.rel_dist(out32, out64)
        shapes_list = np.array([list(v.shape) + [0] * (2 - v.ndim) for v in sd.values()], np.int64)
        np.savez_compressed(os.path.join(OUT, "msda_%s.npz" % tag), shapes=np.array(R.MODULE_LEVELS, np.int64),
                            start=np.array(start, np.int64), query=query, ref=ref, inp=inp,
                            mask=(mask if mask is not None else np.zeros(0, bool)), out32=out32, out64=out64,
                            ref_dist=np.float64(dist), offsets=offsets, logits=logits, state_keys=np.array(list(sd)),
                            state_shapes=shapes_list, **{"sd." + k: v for k, v in sd.items()})
        print("case %s: out %s, reference fp32 distance %.3g" % (tag, out32.shape, dist))


if __name__ == "__main__":
    main()
