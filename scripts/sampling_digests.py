"""sha256 of every raw output tensor of the sampling kernels (mal_costvol.hip, mal_epipolar.hip) over the tests' case tables,
one line per tensor: run it once per library (MAL_HIP_LIB selects another build of the same ABI) and compare the outputs
line by line.  Needs a GPU.

usage: sampling_digests.py > digests.txt

  costvol  the cost-volume sweep's inputs (bin counts, image sizes, frame counts, bin schedules, a dropped sample), filled and
           unfilled, under both values of the option "costvol_impl"
  dyn      DynamicDepth's sweep and golden cases, each under every option route: options off, set_1 and the pooled fill at
           radius 0, 1 and 2, each with and without cv_min
  lookup   the epipolar lookup's case table, forward and all five gradients, under each value of "epi_bwd_planes"
  align    the pose-refinement step's case table piece by piece (plain and robust), forward and all gradients, likewise

A tensor that float atomics sum -- the lookup's d/d fmap1 and d/d fmap2 under "epi_bwd_planes" 0 or where the level planes
exceed the 160 KB of LDS, the align step's d/d tgt under "epi_bwd_planes" 0 or where its plane exceeds 64 KB (ALIGN_LDS_LIMIT
below), and the align step's d/d tgt_w always -- has no fixed summation order: no
library equals itself there from run to run.  Its name carries a ~ and

       sampling_digests.py --compare A.txt B.txt

leaves it out: it prints how many digests were compared, how many of them differ (the gate: none), and how many ~ digests
differ (recorded only; those tensors are held by the tests' oracle gate)."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mal_amd import _lib  # noqa: E402
from oracle import costvol_oracle as CO  # noqa: E402
from tests import costvol_checks, dyn_costvol_restated as R, epipolar_checks as X  # noqa: E402
from tests import test_gpu_costvol_sweep as S, test_gpu_dyn_costvol as DY  # noqa: E402


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def line(tag, tensors):
    print("%-58s | %s" % (tag, " ".join("%s %s" % (k, "-" if v is None else (v if isinstance(v, str) else sha(v)))
                                      for k, v in tensors.items())), flush=True)


def set_option(name, value):
    _lib.check(_lib.load().mal_set_option(name.encode(), int(value)), name)


LDS_LIMIT = 160 * 1024
# the align step's plane kernel also holds a few static LDS bytes; where the runtime then refuses to raise its dynamic limit to
# the device's whole 160 KB the 64 KB default stays in force (plane_lds_limit in mal_epipolar.hip), so a plane above 64 KB may
# take the atomic path: counted as a float-atomic sum
ALIGN_LDS_LIMIT = 64 * 1024


def tagged(tensors, atomic):
    """the names in ``atomic`` get the ~ of a float-atomic sum"""
    return {(k + "~" if k in atomic else k): v for k, v in tensors.items()}


def compare(path_a, path_b):
    a, b = (open(p).read().split("\n") for p in (path_a, path_b))
    assert len(a) == len(b), "the files have %d and %d lines" % (len(a), len(b))
    fixed = differ = atomic = atomic_differ = 0
    for la, lb in zip(a, b):
        if not la and not lb:
            continue
        (ta, fa), (tb, fb) = ((l.split(" | ")[0], l.split(" | ")[1].split()) for l in (la, lb))
        assert ta == tb and fa[0::2] == fb[0::2], (la, lb)
        for name, da, db in zip(fa[0::2], fa[1::2], fb[1::2]):
            if name.endswith("~"):
                atomic, atomic_differ = atomic + 1, atomic_differ + (da != db)
            else:
                fixed, differ = fixed + 1, differ + (da != db)
                if da != db:
                    print("UNEQUAL: %s %s" % (ta.strip(), name))
    print("%d lines, %d digests of fixed-order tensors compared, %d differ; %d digests of float-atomic sums, %d differ"
          % (len([l for l in a if l]), fixed, differ, atomic, atomic_differ))
    return differ


def costvol_cases():
    for D in S.BIN_COUNTS:
        yield "D%d_23x41" % D, S.inputs(2, 2, 23, 41), S.linear(D)
    for h, w in S.SHAPES:
        yield "D11_%dx%d" % (h, w), S.inputs(2, 2, h, w), S.linear(11)
    for F_ in (1, 3, 4):
        yield "F%d_D13_23x41" % F_, S.inputs(2, F_, 23, 41), S.linear(13)
    for binning in ("inverse", "log"):
        yield "%s_D96_24x40" % binning, S.inputs(2, 2, 24, 40), CO.depth_bins(0.5, 20.0, 96, binning)
    cur, look, poses, K, invK = S.inputs(3, 3, 23, 41)
    poses = poses.clone()
    poses[1] = 0.0
    yield "dropped_sample", (cur, look, poses, K, invK), S.linear(13)


def dyn_routes():
    for cv_min in (True, False):
        yield "off_min%d" % cv_min, dict(cv_min=cv_min, set_1=False, pool=False)
        yield "set1_min%d" % cv_min, dict(cv_min=cv_min, set_1=True, pool=False)
        for r in (0, 1, 2):
            yield "pool_r%d_min%d" % (r, cv_min), dict(cv_min=cv_min, set_1=False, pool=True, pool_r=r)


def main():
    names = ("cv", "miss", "masked", "low", "conf")
    for impl in (1, 0):
        set_option("costvol_impl", impl)
        for tag, ins, bins in costvol_cases():
            for fill in (True, False):
                line("costvol impl=%d %s fill=%d" % (impl, tag, fill), dict(zip(names, costvol_checks.run_gpu(*ins, bins, fill))))
    set_option("costvol_impl", 1)

    from mal_amd import costvol
    cases = [(n, R.sweep_case(n)) for n in R.SWEEP] + [(s + "_default", R.load_golden(s + "_default")[0]) for s in R.GOLDEN_SHAPES]
    for name, c in cases:
        for rtag, over in dyn_routes():
            o = dict(DY.opts_of(c), **over)
            cv, miss = costvol.match_features_dynamic(*DY.args_of(c), set_missing_to_max=False, **o)
            outs = costvol.cost_volume_outputs_dynamic(*DY.args_of(c), set_missing_to_max=True, **o)
            line("dyn %s %s" % (name, rtag), dict(zip(names, (cv, miss) + tuple(outs))))

    for planes in (2, 1, 0):
        set_option("epi_bwd_planes", planes)
        for name in X.LOOKUP_CASES:
            c = X.lookup_case(name)
            (B, C, h, w, r, L, heads), _ = X.LOOKUP_CASES[name]
            atomic = ("g_f1", "g_f2") if planes == 0 or X.lookup_lds_bytes(h, w, L) > LDS_LIMIT else ()
            out, grads = X.run_lookup(c)
            line("lookup planes=%d %s" % (planes, name), tagged(dict(out, **{"g_" + k: v for k, v in grads.items()}), atomic))
        for name in X.ALIGN_CASES:
            B, C, h, w = X.ALIGN_CASES[name]
            i = X.align_case(name)
            g = torch.Generator().manual_seed(3)
            w_cp, w_P2 = torch.randn(B, 2, 1, 5, h, w, generator=g), torch.randn(B, 4, h * w, generator=g)
            g_H, g_b = torch.randn(B, 6, 6, generator=g), torch.randn(B, 6, generator=g)
            g_new, g_up = torch.randn(B, 4, 4, generator=g), torch.randn(B, 6, 1, generator=g)
            out, grads = X.run_gradcoords(i, w_cp, w_P2)
            line("align planes=%d %s gradcoords" % (planes, name), dict(out, **{"g_" + k: v for k, v in grads.items()}))
            p2, P2 = X.on_the_robust_bounds(out["c_p"])[0], out["P2"]
            for robust in (False, True):
                atomic = ("g_tgt_w", "g_f2") if planes == 0 or X.align_lds_bytes(h, w) > ALIGN_LDS_LIMIT else ("g_tgt_w",)
                o, gr = X.run_normal_eq(i, p2, P2, g_H, g_b, robust)
                neq = dict(o, **{"g_" + k: v for k, v in gr.items()})
                line("align planes=%d %s normal_eq robust=%d" % (planes, name, robust), tagged(neq, atomic))
                o, gr = X.run_update(neq["H"], neq["b"], i["poses"], g_new, g_up)
                line("align planes=%d %s update robust=%d" % (planes, name, robust), dict(o, **{"g_" + k: v for k, v in gr.items()}))
    set_option("epi_bwd_planes", 2)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--compare"]:
        sys.exit(1 if compare(*sys.argv[2:4]) else 0)
    main()
