"""GPU: the segmenter's two kernel families past the shapes they were merged with -- mal_amd/csrc/mal_msda.hip (above all
the fused route, msda_fwd_kernel<*, true>) and mal_amd/csrc/mal_instances.hip -- on the seeded tables of
tests/segmenter_sweep_cases.py, whose properties tests/test_segmenter_sweep_cases.py proves on the CPU.  The references are
the fp64 checkers tests/msda_restated.py and tests/instances_restated.py; nothing here reads a fixture or the reference tree.

Gates.  MSDA: || hip - c64 ||_2 / || c64 ||_2 <= max(1.25 x own, 1e-6), own = the same distance of the checker evaluated
in fp32 on the same inputs (msda_restated.gate, the clause of test_gpu_msda.py); families M-C and M-E are exact in fp32 in
any order and must be EQUAL to the rounded fp64 checker bit for bit.  Instances: the planes are dyadic, so bytes, classes,
queries and counts must be EQUAL to the checker's and the scores are held to 1e-6 relative against fp64; family I-C orders
by the probability ROUNDED to fp32 (instances_restated.select_fp32), I-D states its own equalities.  Every instances call
goes to the library on buffers filled with a sentinel: a byte outside the planes of the live slots must keep it.
Measured distances: DESIGN.md 13 and 7."""
import ctypes

import numpy as np
import pytest
import torch

from mal_amd import msda
from tests import instances_restated as IR
from tests import msda_restated as MR
from tests import segmenter_sweep_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 1e-6
SENTINEL = 0xAB


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ======================================================================================================================= MSDA
def run_fused(value, levels, start, off, logits, ref, value_dev=None):
    v = dev(value) if value_dev is None else value_dev
    out = msda.ms_deform_attn_fused(v, levels, start, dev(off), dev(logits), dev(ref))
    assert out.dtype == torch.float32 and tuple(out.shape) == (value.shape[0], off.shape[1], value.shape[2] * value.shape[3])
    return out.cpu().numpy()


def run_plain(value, levels, start, loc, weights):
    return msda.ms_deform_attn(dev(value), levels, start, dev(loc), dev(weights)).cpu().numpy()


def both_routes(levels, value, start, off, lg, ref):
    """-> (fused distance, its gate, plain distance, its gate, the two outputs).  The fused route gets the raw inputs; the
    plain route the fp32 checker's own locations and softmax of them, and is held to the operator on those."""
    c64, _, _ = G.fused_chain(value, levels, start, off, lg, ref, np.float64)
    c32, loc32, w32 = G.fused_chain(value, levels, start, off, lg, ref, np.float32)
    fused = run_fused(value, levels, start, off, lg, ref)
    plain = run_plain(value, levels, start, loc32, w32)
    p64 = MR.core(value, levels, start, loc32, w32, np.float64)
    return (MR.rel_dist(fused, c64), MR.gate(MR.rel_dist(c32, c64)), MR.rel_dist(plain, p64), MR.gate(MR.rel_dist(c32, p64)),
            fused, plain)


@pytest.mark.parametrize("L,P", G.MA_LP)
@pytest.mark.parametrize("M,D", G.MA_MD)
def test_ma_both_routes_against_the_checker(M, D, L, P):
    worst = [0.0, 0.0]
    for ref_dim in G.MA_REF_DIMS:
        for N in G.MA_NS:
            for Lq in G.MA_LQS:
                df, gf, dp, gp, _, _ = both_routes(*G.ma_inputs(N, Lq, M, D, L, P, ref_dim))
                worst = [max(worst[0], df), max(worst[1], dp)]
                assert df <= gf, ("fused", ref_dim, N, Lq, df, gf)
                assert dp <= gp, ("plain", ref_dim, N, Lq, dp, gp)
    print("M-A M=%d D=%d L=%d P=%d: largest distance from the fp64 checker fused %.3g plain %.3g" % (M, D, L, P, worst[0], worst[1]))


@pytest.mark.parametrize("ref_dim", G.MA_REF_DIMS)
def test_mb_fused_on_a_value_buffer_off_the_16_byte_grid(ref_dim):
    levels, value, start, off, lg, ref = G.ma_inputs(3, 65, 2, 64, 3, 4, ref_dim)
    aligned = run_fused(value, levels, start, off, lg, ref)
    flat = torch.zeros(value.size + 1, dtype=torch.float32, device=DEV)
    v = flat[1:].view(value.shape)
    v.copy_(dev(value))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    assert G.msda_plan(3, value.shape[1], 65, 2, 64, 3, 4, True)[0] == 4 and G.msda_plan(3, value.shape[1], 65, 2, 64, 3, 4, False)[0] == 1
    assert np.array_equal(bits(run_fused(value, levels, start, off, lg, ref, value_dev=v)), bits(aligned))


@pytest.mark.parametrize("M,D", G.MC_MD)
@pytest.mark.parametrize("ref_dim,L,P", G.MC_CASES)
def test_mc_exact_fused_cases_equal_the_rounded_checker(ref_dim, L, P, M, D):
    levels, value, start, off, lg, ref = G.mc_inputs(ref_dim, L, P, M, D)
    c64, _, _ = G.fused_chain(value, levels, start, off, lg, ref, np.float64)
    out = run_fused(value, levels, start, off, lg, ref)
    assert np.array_equal(bits(out), bits(c64.astype(np.float32)))


@pytest.mark.parametrize("kind", G.MD_KINDS)
@pytest.mark.parametrize("shape", G.MD_SHAPES, ids=str)
def test_md_softmax_extremes(shape, kind):
    levels, value, start, off, lg, ref = G.md_inputs(shape, kind)
    c64, _, _ = G.fused_chain(value, levels, start, off, lg, ref, np.float64)
    c32, _, _ = G.fused_chain(value, levels, start, off, lg, ref, np.float32)
    out = run_fused(value, levels, start, off, lg, ref)
    dist, own = MR.rel_dist(out, c64), MR.rel_dist(c32, c64)
    print("M-D %s %s: kernel distance from fp64 %.3g (fp32 checker's %.3g, gate %.3g)" % (shape, kind, dist, own, MR.gate(own)))
    assert np.isfinite(out).all() and dist <= MR.gate(own)
    if kind == "one_minus_inf":
        # its weight is exactly zero and the rest unchanged: a finite logit whose exponential is zero is the same call
        finite = np.where(np.isneginf(lg), np.float32(-1e30), lg)
        assert np.array_equal(bits(run_fused(value, levels, start, off, finite, ref)), bits(out))
    if kind == "all_1e4":
        uniform = np.zeros_like(lg)
        assert np.array_equal(bits(run_fused(value, levels, start, off, uniform, ref)), bits(out))


@pytest.mark.parametrize("M,D", G.ME_MD)
def test_me_directed_borders_equal_the_rounded_checker(M, D):
    levels, value, start, loc, w = G.me_inputs(M, D)
    c64 = MR.core(value, levels, start, loc, w, np.float64)
    out = run_plain(value, levels, start, loc, w)
    assert np.array_equal(bits(out), bits(c64.astype(np.float32)))
    # each level alone: a sample that one level wrongly admits cannot hide behind the others
    for l in range(len(levels)):
        w1 = np.zeros_like(w)
        w1[:, :, :, l] = w[:, :, :, l]
        want = MR.core(value, levels, start, loc, w1, np.float64).astype(np.float32)
        assert np.array_equal(bits(run_plain(value, levels, start, loc, w1)), bits(want)), levels[l]


def test_mf_the_segmenters_own_table():
    levels, value, start, off, lg, ref = G.mf_inputs()
    df, gf, dp, gp, fused, plain = both_routes(levels, value, start, off, lg, ref)
    print("M-F: distance from the fp64 checker fused %.3g (gate %.3g) plain %.3g (gate %.3g)" % (df, gf, dp, gp))
    assert df <= gf and dp <= gp
    # every output is repeated by a second call
    assert np.array_equal(bits(run_fused(value, levels, start, off, lg, ref)), bits(fused))
    full32 = (MR.locations(off, ref, levels, np.float32), MR.softmax(lg, np.float32).reshape(off.shape[:5]))
    assert np.array_equal(bits(run_plain(value, levels, start, *full32)), bits(plain))


# ================================================================================================================== instances
def run_raw(logits, planes, H, W, T, thing=None):
    """mal_instances on sentinel-filled buffers with one spare mask plane behind the last slot -> per image a dict of numpy
    arrays trimmed to the count.  Asserts that every byte outside the live slots' planes kept the sentinel (a row stored
    past row H-1 of a slot lands in the next plane) and that the slots behind the count hold their defined contents."""
    from mal_amd import _lib as L
    lib = L.load()
    N, Q, K1 = logits.shape
    h, w = planes.shape[2:]
    lg, pm = dev(logits), dev(planes)
    th = None if thing is None else dev(np.asarray(thing, np.uint8))
    ws_bytes = int(lib.mal_instances_workspace_bytes(N, Q, K1 - 1, h, w, H, W, T))
    assert ws_bytes > 0
    masks = torch.full((N * T + 1, H, W), SENTINEL, dtype=torch.uint8, device=DEV)
    classes = torch.full((N, T), -7, dtype=torch.int64, device=DEV)
    f32 = torch.full((3, N, T), -7.0, dtype=torch.float32, device=DEV)
    query = torch.full((N, T), -7, dtype=torch.int32, device=DEV)
    count = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    assert masks.data_ptr() % 4 == 0
    a = L.InstancesArgs()
    a.pred_logits, a.pred_masks, a.thing = lg.data_ptr(), pm.data_ptr(), None if th is None else th.data_ptr()
    a.N, a.Q, a.K, a.h, a.w, a.H, a.W, a.topk = N, Q, K1 - 1, h, w, H, W, T
    a.count, a.masks, a.scores, a.classes, a.query = count.data_ptr(), masks.data_ptr(), f32[0].data_ptr(), classes.data_ptr(), query.data_ptr()
    a.cls_score, a.mask_score = f32[1].data_ptr(), f32[2].data_ptr()
    a.ws, a.ws_bytes, a.stream = ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream
    L.check(lib.mal_instances(ctypes.byref(a)), "mal_instances")
    torch.cuda.synchronize()
    counts = count.cpu().numpy()
    m, cl, f, qu = masks.cpu().numpy(), classes.cpu().numpy(), f32.cpu().numpy(), query.cpu().numpy()
    assert (m[N * T] == SENTINEL).all()
    res = []
    for n in range(N):
        c = int(counts[n])
        assert 0 <= c <= T
        assert (m[n * T + c:(n + 1) * T] == SENTINEL).all(), "image %d: a plane behind slot %d was written" % (n, c - 1)
        assert (cl[n, c:] == 0).all() and (qu[n, c:] == -1).all() and (f[:, n, c:] == 0).all()
        res.append({"pred_masks": m[n * T:n * T + c], "pred_classes": cl[n, :c], "query": qu[n, :c], "scores": f[0, n, :c],
                    "cls_score": f[1, n, :c], "mask_score": f[2, n, :c]})
    return res


def hold(o, c, tag, scores=True):
    """one image's output against the checker's dict: integers equal, scores to FLOOR -> largest score distance"""
    assert np.array_equal(o["query"], c["query"]) and np.array_equal(o["pred_classes"], c["classes"]), tag
    assert set(np.unique(o["pred_masks"]).tolist()) <= {0, 1}, tag
    assert np.array_equal(o["pred_masks"].astype(bool), c["masks"]), tag
    worst = 0.0
    if scores:
        for mine, k in (("cls_score", "cls_score"), ("mask_score", "mask_score"), ("scores", "score")):
            d = IR.rel_dist(o[mine], c[k])
            worst = max(worst, d)
            assert d <= FLOOR, (tag, k, d)
    return worst


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("shape", G.IA_SHAPES, ids=lambda s: "x".join(map(str, s[:4])))
def test_ia_ragged_grids_and_the_cropped_dword_route(shape, N):
    h, w, H, W = shape[:4]
    logits, planes, thing = G.ia_inputs(shape[:4], N)
    out, again = run_raw(logits, planes, H, W, G.IA_T, thing), run_raw(logits, planes, H, W, G.IA_T, thing)
    worst = 0.0
    for n in range(N):
        c = IR.checker(logits[n], planes[n], H, W, G.IA_T, thing)
        worst = max(worst, hold(out[n], c, (shape, n)))
        for k in out[n]:
            assert out[n][k].tobytes() == again[n][k].tobytes(), k
    print("I-A %s N=%d: counts %s, largest score distance from fp64 %.3g" % (shape[:4], N, [len(o["query"]) for o in out], worst))
    # the library's wrapper is the same call
    from mal_amd.instances import instance_inference
    via = instance_inference(dev(logits), dev(planes), (H, W), topk=G.IA_T, thing_classes=None if thing is None else dev(thing))
    for n in range(N):
        assert np.array_equal(via[n]["instances"].pred_masks.cpu().numpy(), out[n]["pred_masks"])
        assert np.array_equal(via[n]["instances"].scores.cpu().numpy(), out[n]["scores"])


@pytest.mark.parametrize("name", G.ib_names())
def test_ib_selection_edges(name):
    Q, K, T, logits, planes, thing = G.ib_inputs(name)
    H, W = G.SMALL_PLANE[2:]
    out = run_raw(logits, planes, H, W, T, thing)
    worst = 0.0
    for n in range(2):
        c = IR.checker(logits[n], planes[n], H, W, T, thing)
        assert len(out[n]["query"]) == len(c["flat"])
        worst = max(worst, hold(out[n], c, (name, n)))
    print("I-B %s: counts %s, largest score distance from fp64 %.3g" % (name, [len(o["query"]) for o in out], worst))


def test_ic_underflowed_probabilities_are_ordered_as_rounded():
    logits, planes = G.ic_inputs()
    H, W = G.SMALL_PLANE[2:]
    out = run_raw(logits, planes, H, W, G.IC_T)
    for n in range(2):
        c = IR.checker(logits[n], planes[n], H, W, G.IC_T, fp32_rule=True)
        o = out[n]
        print("I-C gap %g: device %s, rounded rule %s" % (G.IC_GAPS[n], (o["query"].astype(np.int64) * G.IC_K + o["pred_classes"]).tolist(), c["flat"].tolist()))
        hold(o, c, n, scores=False)
        # the class score IS the rounded probability (a denormal has 12 bits: 1e-6 of it is equality), zero included
        assert IR.rel_dist(o["cls_score"], c["cls_score"]) <= FLOOR
        assert IR.rel_dist(o["mask_score"], c["mask_score"]) <= FLOOR
        # score = cls_score * mask_score in fp32, IEEE: the product of a denormal is rounded on the denormal grid
        assert np.array_equal(bits(o["scores"]), bits(o["cls_score"] * o["mask_score"]))


@pytest.mark.parametrize("exponent", [100, -100])
def test_id_scaled_planes(exponent):
    h, w, H, W = G.ID_SHAPE
    logits, planes = G.id_scaled_inputs(exponent)
    (o,) = run_raw(logits, planes, H, W, G.ID_T)
    c = IR.checker(logits[0], planes[0], H, W, G.ID_T)
    hold(o, c, exponent, scores=False)
    (base,) = run_raw(logits, G.id_scaled_inputs(0)[1], H, W, G.ID_T)
    assert np.array_equal(o["pred_masks"], base["pred_masks"])  # the bytes of the unscaled planes
    assert IR.rel_dist(o["cls_score"], c["cls_score"]) <= FLOOR
    count = c["masks"].reshape(G.ID_T, -1).sum(1).astype(np.float32)
    if exponent > 0:  # every sigmoid is 1: the fp64 sum is the count, and the quotient is the kernel's fp32 one to the bit
        assert np.array_equal(bits(o["mask_score"]), bits(count / (count + np.float32(1e-6))))
    d = IR.rel_dist(o["mask_score"], c["mask_score"])
    print("I-D 2^%d: mask_score distance from fp64 %.3g" % (exponent, d))
    assert d <= FLOOR and IR.rel_dist(o["scores"], c["score"]) <= FLOOR


def test_id_general_planes_under_the_band_rule():
    H, W = G.ID_SHAPE[2:]
    logits, planes = G.id_general_inputs()
    (o,) = run_raw(logits, planes, H, W, G.ID_GENERAL_T)
    c = IR.checker(logits[0], planes[0], H, W, G.ID_GENERAL_T)
    assert np.array_equal(o["query"], c["query"]) and np.array_equal(o["pred_classes"], c["classes"])
    outside, differ, inside = IR.band_report(o["pred_masks"], planes[0][o["query"]], H, W)
    print("I-D general: %d of %d pixels differ from the fp64 rule (%d outside the band), %d inside the band"
          % (differ, G.ID_GENERAL_T * H * W, outside, inside))
    assert outside == 0 and differ <= inside
    for mine, k in (("cls_score", "cls_score"), ("mask_score", "mask_score"), ("scores", "score")):
        assert IR.rel_dist(o[mine], c[k]) <= FLOOR, k
