"""CPU: the restatement of DynamicDepth's hole-aware loss (tests/dyn_loss_restated.py) against the reference's recorded results
(tests/golden/dyn_loss_*.npz, written by scripts/gen_golden_dyn_loss.py from the reference's own Trainer methods), the
admissibility of the case tables tests/test_gpu_dyn_loss.py runs on the device, and the host-side surface: symbols, refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import dyn_loss_restated as R
from tests import operator_checks as X
from tests.epipolar_checks import check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = torch.float64, torch.float32
NEW_SYMBOLS = ("mal_photo_holes_plan", "mal_photo_holes_fwd", "mal_holes_commit", "mal_holes_weight", "mal_photo_holes_bwd")


def bits(t):
    return t.detach().contiguous().numpy().view(np.int32)


def fixture_case(name):
    """the case as the fixture stores it (not as ``golden_case`` would rebuild it) and the recorded results"""
    z = R.load_golden(name)
    B, H, W, scales, over = R.GOLDEN_CASES[name]
    c = dict(name=name, B=B, H=H, W=W, scales=list(scales), over=dict(over))
    c.update({k[3:]: v for k, v in z.items() if k.startswith("in:")})
    return c, z


_SEQ = {}


def sequences(name):
    """float32 and float64 restatement of a fixture's teacher + student sequence, computed once and left unchanged"""
    if name not in _SEQ:
        c, z = fixture_case(name)
        s32 = R.sequence(c, F32)
        _SEQ[name] = (c, z, s32, R.sequence(c, F64, holes=s32["holes"]))
    return _SEQ[name]


@pytest.mark.parametrize("name", sorted(R.GOLDEN_CASES))
def test_restatement_equals_the_reference_bit_for_bit(name):
    c, z, s32, _ = sequences(name)
    rebuilt = R.golden_case(name)
    for k, v in rebuilt.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, c[k]), (name, "golden_case no longer builds the fixture's input", k)
    n = 0
    for tag in ("t", "s"):
        for k in [k for k in z if k.startswith("loss_%s:" % tag)]:
            assert np.array_equal(bits(z[k]), bits(s32["losses_" + tag][k.split(":", 1)[1]])), (name, k)
            n += 1
        assert np.array_equal(bits(z["target_" + tag]), bits(s32["target_" + tag])), (name, tag, "mutated target")
        for s in c["scales"]:
            for i in range(2):
                assert torch.equal(z["holes_%s/%d/%d" % (tag, s, i)], s32["recs_" + tag][s]["first"]["holes"][i]), (name, tag, s, i)
    for s in c["scales"]:
        assert np.array_equal(bits(z["consistency_target/%d" % s]), bits(s32["losses_s"]["consistency_target/%d" % s]))
    assert n == 2 * (2 * len(c["scales"]) + 1) + len(c["scales"])      # reproj, loss per scale, loss; consistency for the student
    for k in R.LEAVES:
        for kk in [x for x in s32["grads"] if x == k or x.startswith(k + "/")]:
            g = z["grad:" + kk]
            assert float((g - s32["grads"][kk]).abs().max()) <= 1e-6 * float(g.abs().max()) + 1e-12, (name, kk)
    if c["over"].get("zero_img", True):   # the carried-over zeroing is in the data: the student zeroes further
        zt, zs = (z["target_t"].sum(1) == 0), (z["target_s"].sum(1) == 0)
        assert int(zt.sum()) > 0 and int(zs.sum()) > int(zt.sum()) and bool((zs | ~zt).all())
    else:
        assert torch.equal(z["target_t"], c["color0"]) and torch.equal(z["target_s"], c["color0"])


@pytest.mark.parametrize("name", sorted(R.GOLDEN_CASES))
def test_fixture_rows_hold_every_hole_category(name):
    c, z = fixture_case(name)
    s0 = c["scales"][0]
    for tag in ("t", "s"):
        cat = R.hole_categories([z["holes_%s/%d/%d" % (tag, s0, i)] for i in range(2)])
        assert min(cat.values()) > 0, (name, tag, cat)


@pytest.mark.parametrize("name", sorted(R.GOLDEN_CASES))
def test_fixture_cases_are_admissible(name):
    """float32 against float64: decisions differ at no more than decision_cap(N) pixels, each a near-tie; the hole bytes are
    the same (taken from the float32 candidates); the float32 values pass the gate's floor"""
    c, z, s32, s64 = sequences(name)
    # the values are compared as the device's will be: on the same decisions (here float64's own, forced on float32)
    forced = {(tag == "s", s): dict(choice=s64["recs_" + tag][s]["first"]["choice"], weight=s64["recs_" + tag][s]["weight"])
              for tag in ("t", "s") for s in c["scales"]}
    forced32 = R.sequence(c, F32, holes=s32["holes"], forced=forced)
    for tag in ("t", "s"):
        for s in c["scales"]:
            a, b = s32["recs_" + tag][s], s64["recs_" + tag][s]
            for i in range(2):
                assert torch.equal(a["first"]["holes"][i], b["first"]["holes"][i])
                if a["ident"] is not None:
                    assert torch.equal(a["ident"]["holes"][i], b["ident"]["holes"][i])
            X.hold_decisions(a["first"]["choice"], b["first"]["choice"], b["first"]["margin_min"], "%s %s/%d argmin" % (name, tag, s))
            if b["margin_mask"] is not None:
                X.hold_decisions(a["weight"], b["weight"].float(), b["margin_mask"], "%s %s/%d automask" % (name, tag, s))
            else:
                assert torch.equal(a["weight"].double(), b["weight"])
        l32 = {k: v.detach().reshape(1) for k, v in forced32["losses_" + tag].items() if v.dim() == 0}
        l64 = {k: v.detach().reshape(1) for k, v in s64["losses_" + tag].items() if v.dim() == 0}
        check(l32, l64, None, forward=True, floor=1e-4, what="%s %s" % (name, tag))


@pytest.mark.parametrize("name", sorted(R.SWEEP_CASES))
def test_sweep_cases_are_admissible(name):
    c = R.sweep_case(name)
    kw = dict(ident=c["ident"], noise=c["noise"], ext=c["ext"])
    hs = [R.hole_bytes(x) for x in c["cands"]]
    o64, g64 = R.photo_holes_grads(c["target"], c["cands"], c["flags"], F64, scale=c["scale"], holes=hs, **kw)
    own32 = R.photo_holes(c["target"], c["cands"], c["flags"], F32, **kw)
    X.hold_decisions(own32["choice"], o64["choice"], o64["margin_min"], name + " argmin")
    if o64["margin_mask"] is not None:
        X.hold_decisions(own32["weight"], o64["weight"].float(), o64["margin_mask"], name + " automask")
    forced = dict(choice=o64["choice"], weight=o64["weight"])
    o32, g32 = R.photo_holes_grads(c["target"], c["cands"], c["flags"], F32, scale=c["scale"], holes=hs, forced=forced, **kw)
    check(dict(rp=o32["rp"].detach(), s=o32["sums"][:1].detach()), dict(rp=o64["rp"].detach(), s=o64["sums"][:1].detach()), None,
          forward=True, floor=1e-4, what=name)
    ex = R.ssim_exempt_holes(o64, c["target"], c["cands"], c["flags"]).expand(-1, 3, -1, -1)
    check(X.masked({"g%d" % i: g for i, g in enumerate(g32)}, ex), X.masked({"g%d" % i: g for i, g in enumerate(g64)}, ex), None,
          numel=o64["rp"].numel(), floor=1e-4, what=name + " grads")
    # what the row claims
    B, H, W, n, flags, opts = R.SWEEP_CASES[name]
    cat = R.hole_categories(hs)
    if opts.get("all_hole"):
        assert cat["none"] == 0 and (cat["both"] if n == 2 else cat["h0_only"]) == B * H * W
    elif opts.get("no_hole"):
        assert cat["none"] == B * H * W
    elif n == 2:
        assert min(cat.values()) > 0, (name, cat)
        one_px = hs[0][:, H // 2, W // 2] & ~hs[0][:, H // 2, W // 2 - 1] & ~hs[0][:, H // 2, W // 2 + 1]
        assert one_px.all() or H < 7                                     # the one-pixel hole
        full = torch.nn.functional.avg_pool2d(hs[1].float().unsqueeze(1), 3, 1)
        assert float(full.max()) == 1.0                                  # a hole whose whole 3x3 neighbourhood is hole
    else:
        assert cat["h0_only"] > 0 and cat["none"] > 0
    if not (opts.get("all_hole") or opts.get("no_hole")) and H >= 5:      # the soft edge: channel sums on both sides of 0.1
        sums = torch.cat([x.sum(1).flatten() for x in c["cands"]])
        assert int(((sums > 0) & (sums < 0.1)).sum()) > 0 and int(((sums >= 0.1) & (sums < 0.18)).sum()) > 0


def test_sweep_shapes_cover_what_the_kernel_branches_on():
    shapes = {(B, H, W) for B, H, W, _, _, _ in R.SWEEP_CASES.values()}
    assert {(1, 2, 2), (1, 5, 7), (1, 9, 63), (1, 9, 64), (3, 9, 65), (1, R.TILE_H, R.TILE_W), (3, R.TILE_H + 1, R.TILE_W + 1)} <= shapes
    combos = {(n, fl) for _, _, _, n, fl, _ in R.SWEEP_CASES.values()}
    for n in (1, 2):   # the full product of the five flags (SELECT is refused at n = 1), with and without ext_mask among them
        want = R.flag_product(n)
        assert len(want) == (32 if n == 2 else 16) and len(set(want)) == len(want)
        assert {(n, fl) for fl in want} <= combos, sorted({(n, fl) for fl in want} - combos)
    rows = [(fl, bool(o.get("ext"))) for k, (_, _, _, _, fl, o) in R.SWEEP_CASES.items() if k.startswith("flags_n")]
    assert (0, True) in rows                                             # flags off, with ext_mask
    for f, _ in R.FLAG_NAMES:                                            # every flag runs with and without ext_mask
        assert {e for fl, e in rows if fl & f} == {True, False}


def test_new_symbols_are_declared_bound_and_exported():
    from mal_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "mal_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "mal_holes.hip" in build.SOURCES
    build.build(verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert n in _lib.SIGNATURES and hasattr(raw, n), n
    assert (_lib.F_ZERO_IMG, _lib.F_SELECT) == (R.F_ZERO_IMG, R.F_SELECT) == (512, 1024)
    assert re.search(r"MAL_F_ZERO_IMG\s*=\s*512", header) and re.search(r"MAL_F_SELECT\s*=\s*1024", header)
    assert (_lib.HOLE_CHOICE_NONE, _lib.HOLE_CHOICE_AVG) == (R.CHOICE_NONE, R.CHOICE_AVG)


def test_library_refuses_by_code_before_any_device_work():
    from mal_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    n = None
    two = _lib.ptr_array([None, None])
    fwd = lambda nc, H, W, fl: lib.mal_photo_holes_fwd(n, two, nc, n, n, n, 1, H, W, fl, n, n, n, n, n, n, 0, n)
    assert fwd(3, 8, 8, 0) == -1 and fwd(0, 8, 8, 0) == -1                 # n_cand outside 1..2
    assert fwd(1, 8, 8, _lib.F_SELECT) == -1                              # SELECT needs exactly two
    assert fwd(2, 1, 8, 0) == -1 and fwd(2, 8, 1, 0) == -1                # H or W < 2: MAL_EINVAL here
    assert fwd(2, 8, 8, _lib.F_GRAD) == -1 and fwd(2, 8, 8, 0) == -1      # another entry point's flag; null pointers
    assert lib.mal_holes_commit(n, n, 2, 1, 8, 8, n) == -1 and lib.mal_holes_commit(n, n, 3, 1, 8, 8, n) == -1
    assert lib.mal_photo_holes_bwd(n, two, 3, n, n, n, n, n, 1, 8, 8, 0, two, n) == -1
    assert lib.mal_photo_holes_bwd(n, two, 1, n, n, n, n, n, 1, 8, 8, _lib.F_SELECT, two, n) == -1
    assert lib.mal_holes_weight(n, n, n, n, 1, 8, 8, n, n, n, 0, n) == -1
    iv = [ctypes.c_int() for _ in range(5)]
    lds = [ctypes.c_size_t() for _ in range(2)]
    args = [ctypes.byref(v) for v in iv + lds]
    assert lib.mal_photo_holes_plan(1, 1, 8, *args) == -1
    assert lib.mal_photo_holes_plan(3, R.TILE_H + 1, R.TILE_W + 1, *args) == 0
    assert [v.value for v in iv] == [R.TILE_W, R.TILE_H, 1, 2, 12]


def test_python_surface_refuses_by_name():
    from mal_amd import _lib, dyn_loss, ops
    t = torch.zeros(1, 3, 8, 8)
    with pytest.raises(_lib.MalError, match="1 or 2 candidates"):
        ops.photo_holes_fwd(t, [t, t, t])
    with pytest.raises(_lib.MalError, match="exactly two"):
        ops.photo_holes_fwd(t, [t], flags=_lib.F_SELECT)
    with pytest.raises(_lib.MalError, match="does not match"):
        ops.photo_holes_fwd(t, [t, torch.zeros(1, 3, 8, 9)])
    with pytest.raises(_lib.MalError, match="H, W >= 2"):
        ops.photo_holes_fwd(torch.zeros(1, 3, 1, 8), [torch.zeros(1, 3, 1, 8)])
    with pytest.raises(_lib.MalError, match="CUDA/HIP"):                  # no CPU fallback
        ops.photo_holes_fwd(t, [t, t], flags=_lib.F_ZERO_IMG)
    lp = dyn_loss.LossPath(dyn_loss.default_options(v1_multiscale=True))
    for call in (lambda: lp.generate_images_pred({}, {}), lambda: lp.compute_losses({}, {})):
        with pytest.raises(NotImplementedError, match="v1_multiscale") as e:
            call()
        assert "dynamicdepth/trainer.py:" in str(e.value)
    lp = dyn_loss.LossPath(dyn_loss.default_options(feat_loss="true"))   # refused where upstream would call the missing function
    with pytest.raises(NotImplementedError, match="feat_loss") as e:
        lp.compute_losses({}, {}, is_multi=True)
    assert "dynamicdepth/trainer.py:" in str(e.value)
    lp = dyn_loss.LossPath(dyn_loss.default_options(frame_ids=[0, -1]))
    with pytest.raises(_lib.MalError, match="selec_reproj"):
        lp.compute_losses({}, {})
