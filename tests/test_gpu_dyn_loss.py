"""DynamicDepth's hole-aware reprojection loss on the device (mal_amd/csrc/mal_holes.hip through mal_amd.ops, mal_amd.functional
and mal_amd.dyn_loss) against tests/dyn_loss_restated.py.

The gate is ``epipolar_checks.check`` unchanged, as tests/test_gpu_operator_sweep.py uses it for ``photo_fwd``: floor 1e-4 (what
tests/test_gpu_layers.py asserts for the same arithmetic) or 1.25 x the float32 restatement's own distance from float64;
per-pixel gradient maps with the allowance 2e-4 + 4/numel; SSIM's clamp exempt as ``operator_checks.ssim_exempt``.  The hole
bytes and the committed target are BITWISE the restatement's; the device's choice and weight are forced on the float64
restatement and may differ from its own at no more than ``decision_cap(N)`` pixels, each a near-tie (<= 1e-4).
"""
import pytest
import torch

from tests import dyn_loss_restated as R
from tests import operator_checks as X
from tests.epipolar_checks import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


def dev(t):
    if isinstance(t, (list, tuple)):
        return [dev(x) for x in t]
    return None if t is None else t.to(DEV)


def cpu(t):
    if isinstance(t, (list, tuple)):
        return [cpu(x) for x in t]
    return None if t is None else t.detach().cpu()


def pixel_route():
    """context manager: mal_photo_fwd / _bwd on their one-pixel-per-thread kernels (ATen's summation order)"""
    from tests.test_gpu_operator_sweep import options
    return options(photo_impl=0)


def run_device(c, need=None):
    """forward, commit, backward of one case -> CPU tensors.  The backward gets the copy of the target taken before the commit."""
    from mal_amd import ops
    tgt, cands = dev(c["target"].clone()), dev(c["cands"])
    seen = tgt.clone()
    holes, mn, ch, wt, sums = ops.photo_holes_fwd(tgt, cands, dev(c["ident"]), dev(c["noise"]), dev(c["ext"]), c["flags"])
    assert torch.equal(tgt, seen), "the forward wrote the target"
    if c["flags"] & R.F_ZERO_IMG:
        ops.holes_commit(tgt, holes)
    scale = torch.tensor([c["scale"]], device=DEV)
    g = ops.photo_holes_bwd(seen, cands, holes, ch, wt, scale, sums, c["flags"], need or [True] * len(cands))
    torch.cuda.synchronize()
    return dict(holes=cpu(holes), mn=cpu(mn), ch=cpu(ch), wt=cpu(wt), sums=cpu(sums), target_after=cpu(tgt), grads=cpu(g))


def gate_case(c, d, what):
    """the operator gate of one case ``c`` on the device's results ``d``"""
    n, flags = len(c["cands"]), c["flags"]
    kw = dict(ident=c["ident"], noise=c["noise"], ext=c["ext"])
    own32 = R.photo_holes(c["target"], c["cands"], flags, F32, **kw)
    hs = own32["holes"]
    # bitwise: the hole bytes and the committed target
    for k in range(n):   # (without a hole flag the test is not taken: the bytes are 0)
        assert torch.equal(d["holes"][k].bool(), hs[k] if flags & R.ZS else torch.zeros_like(hs[k])), (what, "hole bytes", k)
    assert torch.equal(d["target_after"], own32["target_after"]), (what, "committed target")
    assert torch.equal(d["target_after"] == 0, own32["target_after"] == 0)
    # decisions: the device's against the float64 restatement's own
    own64 = R.photo_holes(c["target"], c["cands"], flags, F64, holes=hs, **kw)
    N = d["ch"].numel()
    X.hold_decisions(d["ch"].long(), own64["choice"], own64["margin_min"], what + " choice")
    if flags & R.F_AUTOMASK:
        X.hold_decisions(d["wt"], own64["weight"].float(), own64["margin_mask"], what + " weight")
    else:
        assert torch.equal(d["wt"], own64["weight"].float()), (what, "weight")
    assert float(d["sums"][1]) == float(d["wt"].double().sum())      # 0/1 weights: exact
    # values and gradients with the device's decisions forced
    forced = dict(choice=d["ch"], weight=d["wt"])
    refs = []
    for dt in (F64, F32):
        out, g = R.photo_holes_grads(c["target"], c["cands"], flags, dt, scale=c["scale"], holes=hs, forced=forced, **kw)
        refs.append((dict(min_reproj=out["rp"].detach(), sum_rw=out["sums"][:1].detach()),
                     {"g_cand%d" % k: g[k] for k in range(n)}, out))
    (o64, g64, full64), (o32, g32, _) = refs
    print(what, check(dict(min_reproj=d["mn"], sum_rw=d["sums"][:1]), o64, o32, forward=True, floor=1e-4, what=what))
    ex = R.ssim_exempt_holes(full64, c["target"], c["cands"], flags).expand(-1, 3, -1, -1)
    got = X.masked({"g_cand%d" % k: d["grads"][k] for k in range(n)}, ex)
    print(what, check(got, X.masked(g64, ex), X.masked(g32, ex), numel=N, floor=1e-4, what=what + " grads"))
    return hs


def test_plan_reports_the_tile_the_cases_are_built_for():
    from mal_amd import ops
    p = ops.photo_holes_plan(3, 9, 33)
    assert (p["tile_w"], p["tile_h"], p["halo_fwd"], p["halo_bwd"]) == (R.TILE_W, R.TILE_H, 1, 2)
    assert p["blocks"] == 3 * 2 * 2 and ops.photo_holes_plan(1, 8, 32)["blocks"] == 1
    assert p["lds_fwd"] < p["lds_bwd"] < 64 * 1024


@pytest.mark.parametrize("name", sorted(R.SWEEP_CASES))
def test_operator_gate_over_the_sweep(name):
    c = R.sweep_case(name)
    d = run_device(c)
    hs = gate_case(c, d, name)
    d2 = run_device(c)                                                     # two runs are equal
    for k in ("holes", "mn", "ch", "wt", "sums", "target_after"):
        assert torch.equal(d[k], d2[k]), (name, k)
    for a, b in zip(d["grads"], d2["grads"]):
        assert torch.equal(a, b), name
    if c["flags"] & R.F_ZERO_IMG:                                          # the gradient at every h_c pixel of P_c is exactly 0
        for k, g in enumerate(d["grads"]):
            assert float(g[hs[k].unsqueeze(1).expand_as(g)].abs().sum()) == 0.0, (name, k)
    if (c["flags"] & R.ZS) == R.ZS and len(hs) == 2:                       # a both-hole pixel: rp = 0, nothing flows
        both = (hs[0] & hs[1]).unsqueeze(1)
        assert torch.equal(d["ch"][both], torch.full_like(d["ch"][both], R.CHOICE_NONE))
        assert float(d["mn"][both].abs().sum()) == 0.0
        for g in d["grads"]:
            assert float(g[both.expand_as(g)].abs().sum()) == 0.0


def test_sweep_cases_hold_what_they_claim():
    """the categories the sweep is there for are in its data (the CPU file asserts the same of the fixtures)"""
    c = R.sweep_case("b3_9x33_across_the_tile")
    hs = [R.hole_bytes(x) for x in c["cands"]]
    cat = R.hole_categories(hs)
    assert min(cat.values()) > 0, cat
    assert hs[0][:, :2, :2].all() and hs[1][:, -2:, -2:].all()               # holes on the image border, in two corners
    assert hs[0][:, R.TILE_H - 1:R.TILE_H + 1, R.TILE_W - 1:R.TILE_W + 1].all()   # across both tile seams


@pytest.mark.parametrize("name", ["b1_17x40_flags_off", "b1_17x40_n1_flags_off_automask", "b1_17x40_avg_no_select",
                                  "b1_12x35_n1_no_ssim_avg"])
@pytest.mark.parametrize("how", ["flags_off", "flags_on_no_pixel_under_the_threshold"])
def test_without_holes_the_outputs_are_photo_fwd_and_bwd_bit_for_bit(name, how):
    """Same arithmetic in the same order as the one-pixel-per-thread kernels of mal_photo.hip (photo_impl = 0; the marching
    default reassociates the window sums).  The sums are compared bitwise too: rp * w are float32 values in [0, 1]
    over a few hundred pixels, so every partial sum is exact in float64 whatever the order."""
    from mal_amd import ops
    c = R.sweep_case(name)
    base = c["flags"] & (R.F_AUTOMASK | R.F_AVG | R.F_NO_SSIM)
    if how == "flags_off":
        c["flags"] = base
    else:
        for x in c["cands"]:   # repaint: no hole anywhere (every channel >= 0.06: the sums are >= 0.18)
            x.clamp_(min=0.06)
        c["flags"] = base | R.F_ZERO_IMG | (R.F_SELECT if len(c["cands"]) == 2 else 0)
        assert not any(R.hole_bytes(x).any() for x in c["cands"])
    d = run_device(c)
    assert torch.equal(d["target_after"], c["target"]), "the target was touched"
    with pixel_route():
        tgt, cands = dev(c["target"]), dev(c["cands"])
        mn, am, wt, sums = ops.photo_fwd(tgt, cands, dev(c["ident"]), dev(c["noise"]), dev(c["ext"]), base)
        g = ops.photo_bwd(tgt, cands, am, wt, torch.tensor([c["scale"]], device=DEV), sums, base & ~R.F_AUTOMASK, [True] * len(cands))
        torch.cuda.synchronize()
    assert torch.equal(d["mn"], cpu(mn)) and torch.equal(d["ch"], cpu(am)) and torch.equal(d["wt"], cpu(wt))
    assert torch.equal(d["sums"][:2], cpu(sums)[:2])
    for a, b in zip(d["grads"], cpu(g)):
        assert torch.equal(a, b)


def test_backward_after_the_target_was_zeroed_further():
    """teacher forward, then the student forward on the same target (which zeroes it further), then both backwards: each uses
    the target as it was at ITS evaluation"""
    from mal_amd import functional as Fn
    c1 = R.sweep_case("b3_9x33_across_the_tile")
    target = c1["target"]
    a = [x.clone() for x in c1["cands"]]
    b = [x.flip(-1).contiguous() for x in c1["cands"]]     # the second call's holes lie elsewhere: it zeroes the target further
    flags = R.ZS
    tgt = dev(target.clone())
    la = [x.to(DEV).requires_grad_(True) for x in a]
    lb = [x.to(DEV).requires_grad_(True) for x in b]
    l1, _, w1, h1, ch1, t1 = Fn.HolePhotoLossFn.apply(tgt, None, None, flags, False, 0, *la)
    after1 = t1.detach().clone()
    l2, _, w2, h2, ch2, t2 = Fn.HolePhotoLossFn.apply(t1, None, None, flags, False, 0, *lb)
    assert t2.data_ptr() == tgt.data_ptr() and not t2.requires_grad and t2.grad_fn is None
    (0.7 * l1 + 1.3 * l2).backward()
    torch.cuda.synchronize()
    r1 = R.photo_holes(target, a, flags, F32)
    r2 = R.photo_holes(r1["target_after"], b, flags, F32)
    assert torch.equal(cpu(after1), r1["target_after"]) and torch.equal(cpu(t2), r2["target_after"])
    assert int((r2["target_after"] != r1["target_after"]).sum()) > 0
    N = w1.numel()
    for cands, leaves, tg, ch, w, k, what in ((a, la, target, ch1, w1, 0.7, "first"), (b, lb, r1["target_after"], ch2, w2, 1.3, "second")):
        forced = dict(choice=cpu(ch), weight=cpu(w))
        (o64, g64), (o32, g32) = (R.photo_holes_grads(tg, cands, flags, dt, scale=k, forced=forced) for dt in (F64, F32))
        ex = R.ssim_exempt_holes(o64, tg, cands, flags).expand(-1, 3, -1, -1)
        got = X.masked({"g%d" % i: cpu(x.grad) for i, x in enumerate(leaves)}, ex)
        check(got, X.masked({"g%d" % i: g for i, g in enumerate(g64)}, ex), X.masked({"g%d" % i: g for i, g in enumerate(g32)}, ex),
              numel=N, floor=1e-4, what=what)
    # ... and a backward that read the caller's target of now would not pass: the first call's windows changed
    wrong = R.photo_holes_grads(r2["target_after"], a, flags, F64, scale=0.7, forced=dict(choice=cpu(ch1), weight=cpu(w1)))[1]
    right = R.photo_holes_grads(target, a, flags, F64, scale=0.7, forced=dict(choice=cpu(ch1), weight=cpu(w1)))[1]
    assert float((wrong[0] - right[0]).abs().max()) > 1e-3 * float(right[0].abs().max())


def test_captured_forward_and_commit_follow_rewritten_candidates():
    from mal_amd import ops
    c = R.sweep_case("b3_9x33_across_the_tile")
    alt = [x.flip(-1).contiguous() for x in c["cands"]]
    tgt0 = dev(c["target"])
    tgt, cands = tgt0.clone(), [x.clone() for x in dev(c["cands"])]
    ident, noise, ext = dev(c["ident"]), dev(c["noise"]), dev(c["ext"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up on the capturing stream: the workspace exists before capture
        ops.photo_holes_fwd(tgt, cands, ident, noise, ext, c["flags"])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = ops.photo_holes_fwd(tgt, cands, ident, noise, ext, c["flags"])
        ops.holes_commit(tgt, out[0])
    for images in (c["cands"], alt):
        for dst, src in zip(cands, images):
            dst.copy_(src.to(DEV))
        tgt.copy_(tgt0)
        graph.replay()
        torch.cuda.synchronize()
        t2 = tgt0.clone()
        want = ops.photo_holes_fwd(t2, dev(images), ident, noise, ext, c["flags"])
        ops.holes_commit(t2, want[0])
        torch.cuda.synchronize()
        for a, b in zip(out, want):
            assert torch.equal(a[:2] if a.dtype == F64 else a, b[:2] if b.dtype == F64 else b)
        assert torch.equal(tgt, t2)


def test_refusals():
    from mal_amd import _lib as L, ops
    lib = L.load()
    t = torch.zeros(1, 3, 4, 4, device=DEV)
    ws = ops.workspace(t.device, 1, 4, 4)
    ptrs = L.ptr_array([t.data_ptr()] * 3)
    hb = torch.zeros(3, 1, 4, 4, dtype=torch.uint8, device=DEV)
    sums = torch.zeros(8, dtype=F64, device=DEV)
    call = lambda n, H, W, fl: lib.mal_photo_holes_fwd(t.data_ptr(), ptrs, n, None, None, None, 1, H, W, fl, hb.data_ptr(), None, None,
                                                       None, sums.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert call(3, 4, 4, 0) == -1 and call(3, 4, 4, L.F_SELECT) == -1           # n <= 2
    assert call(1, 4, 4, L.F_SELECT) == -1                                      # SELECT needs two
    assert call(2, 1, 4, 0) == -1 and call(2, 4, 1, 0) == -1                    # H, W >= 2
    assert call(2, 4, 4, L.F_GRAD) == -1                                        # a flag of another entry point
    assert lib.mal_photo_holes_fwd(t.data_ptr(), ptrs, 2, None, None, None, 1, 4, 4, L.F_AUTOMASK, hb.data_ptr(), None, None, None,
                                   sums.data_ptr(), ws.data_ptr(), ws.numel(), None) == -1     # automask without ident
    assert lib.mal_holes_commit(t.data_ptr(), hb.data_ptr(), 3, 1, 4, 4, None) == -1
    with pytest.raises(L.MalError, match="does not match"):
        ops.photo_holes_fwd(t, [t, torch.zeros(1, 3, 4, 5, device=DEV)], flags=L.F_ZERO_IMG)
    with pytest.raises(L.MalError, match="exactly two"):
        ops.photo_holes_fwd(t, [t], flags=L.F_SELECT)
    with pytest.raises(L.MalError, match="ident"):
        ops.photo_holes_fwd(t, [t, t], flags=L.F_AUTOMASK)


# ================================================================ the loss path against the fixtures
def device_sequence(c, opt_over=None, path="dyn"):
    """the teacher's generate_images_pred + compute_losses, then the student's, on the SAME inputs dictionary, through
    ``mal_amd.dyn_loss.LossPath`` (or, ``path="mal"``, ``mal_amd.trainer.LossPath``'s operator route) -> losses, targets after each
    pass, leaf gradients of losses_t['loss'] + losses_s['loss'], the decisions per (is_multi, scale)"""
    from mal_amd import dyn_loss, trainer
    over = dict(c["over"], **(opt_over or {}))
    B, H, W, scales = c["B"], c["H"], c["W"], c["scales"]
    if path == "dyn":
        lp = dyn_loss.LossPath(dyn_loss.default_options(height=H, width=W, batch_size=B, scales=list(scales), **over))
    else:
        lp = trainer.LossPath(trainer.default_options(height=H, width=W, batch_size=B, sclm=0, distil=False), fuse=False)
    inputs = {("color", 0, 0): dev(c["color0"].clone()), ("K", 0): dev(c["K"]), ("inv_K", 0): dev(c["inv_K"])}
    for s in scales:
        if s:
            inputs[("color", 0, s)] = dev(c["color0/%d" % s])
    for f, tag in ((-1, "m1"), (1, "p1")):
        inputs[("color", f, 0)], inputs[("ori_color", f, 0)] = dev(c["color_" + tag]), dev(c["ori_" + tag])
    lv = {k: dev(c[k]).clone().requires_grad_(True) for k in c if k.startswith(("disp_t/", "disp_s/")) or k in ("T_m1", "T_p1")}
    res, depth_t, decisions = {}, {}, {}
    for is_multi, tag in ((False, "t"), (True, "s")):
        outputs = {("cam_T_cam", 0, -1): lv["T_m1"], ("cam_T_cam", 0, 1): lv["T_p1"]}
        for s in scales:
            outputs[("disp", s)] = lv["disp_%s/%d" % (tag, s)]
        if is_multi:
            outputs["consistency_mask"], outputs["augmentation_mask"] = dev(c["consistency_mask"]), dev(c["augmentation_mask"])
            for s in scales:
                outputs[("mono_depth", 0, s)] = depth_t[s].detach()
        lp.generate_images_pred(inputs, outputs, is_multi=is_multi)
        noise = {s: dev(c["noise_%s/%d" % (tag, s)]) for s in scales}
        if path == "dyn":
            losses = lp.compute_losses(inputs, outputs, is_multi=is_multi, noise=noise)
        else:
            losses, _ = lp.compute_losses(inputs, outputs, is_multi=is_multi, noises=noise)
        for s in scales:
            depth_t[s] = outputs[("depth", 0, s)]
            if path == "dyn":
                decisions[(is_multi, s)] = {k: cpu(outputs[("hole_" + k, s)]) for k in ("choice", "weight", "mask")}
            if is_multi and "consistency_target/%d" % s in outputs:
                losses["consistency_target/%d" % s] = outputs["consistency_target/%d" % s]
        res["losses_" + tag] = losses
        res["target_" + tag] = cpu(inputs[("color", 0, 0)].clone())
    (res["losses_t"]["loss"] + res["losses_s"]["loss"]).backward()
    torch.cuda.synchronize()
    res["grads"] = {k: cpu(v.grad) if v.grad is not None else torch.zeros_like(c[k]) for k, v in lv.items()}
    assert not inputs[("color", 0, 0)].requires_grad and inputs[("color", 0, 0)].grad_fn is None   # still the plain input tensor
    res["decisions"] = decisions
    for tag in ("t", "s"):
        res["losses_" + tag] = {k: cpu(v) for k, v in res["losses_" + tag].items()}
    return res


@pytest.mark.parametrize("name", sorted(R.GOLDEN_CASES))
def test_compute_losses_against_the_fixtures(name):
    from tests.test_dyn_loss_cases import fixture_case
    c, z = fixture_case(name)
    d = device_sequence(c)
    # the targets each pass leaves and the hole bytes: bitwise the reference's
    for tag in ("t", "s"):
        assert torch.equal(d["target_" + tag], z["target_" + tag]), (name, tag, "mutated target")
        for s in c["scales"]:
            hb = d["decisions"][(tag == "s", s)]["mask"]
            want = [z["holes_%s/%d/%d" % (tag, s, i)] for i in range(2)]
            for i in range(2):
                assert torch.equal(hb[i].bool(), want[i] if R.flags_of(R.opt_of(c)) & R.ZS else torch.zeros_like(want[i])), (name, tag, s, i)
    # decisions: the device's against float64's own; then forced on both restatements
    s32 = R.sequence(c, F32)
    s64 = R.sequence(c, F64, holes=s32["holes"])
    N = c["B"] * c["H"] * c["W"]
    for tag in ("t", "s"):
        for s in c["scales"]:
            dec, rec = d["decisions"][(tag == "s", s)], s64["recs_" + tag][s]
            X.hold_decisions(dec["choice"].long(), rec["first"]["choice"], rec["first"]["margin_min"], "%s %s/%d choice" % (name, tag, s))
            if rec["margin_mask"] is not None:
                X.hold_decisions(dec["weight"], rec["weight"].float(), rec["margin_mask"], "%s %s/%d weight" % (name, tag, s))
            else:
                assert torch.equal(dec["weight"].double(), rec["weight"])
    forced = {k: dict(choice=v["choice"], weight=v["weight"]) for k, v in d["decisions"].items()}
    f64, f32 = (R.sequence(c, dt, holes=s32["holes"], forced=forced) for dt in (F64, F32))
    for tag in ("t", "s"):
        for k, v in f64["losses_" + tag].items():
            got = d["losses_" + tag][k].double()
            ref = v.detach()
            err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
            print(name, tag, k, "device %.3e" % err, "float32 restatement %.3e" % (
                float((f32["losses_" + tag][k].detach().double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)))
            assert err <= 1e-5, (name, tag, k, err)
    print(name, check(d["grads"], f64["grads"], f32["grads"], numel=N, floor=1e-4, what=name + " leaf gradients"))


@pytest.mark.parametrize("name", ["b2_12x20_both_off", "b1_9x70_both_off"])
def test_with_both_options_off_the_path_is_manydepths(name):
    """zero_img and selec_reproj off (and the teacher on the frames the student sees): ``MALLossPath``'s operator route on the
    same inputs, bit for bit under photo_impl = 0 -- the same arithmetic in the same order"""
    from tests.test_dyn_loss_cases import fixture_case
    c, _ = fixture_case(name)
    with pixel_route():
        a = device_sequence(c, dict(no_teacher_warp=False))
        b = device_sequence(c, path="mal")
    for tag in ("t", "s"):
        assert torch.equal(a["target_" + tag], c["color0"]) and torch.equal(b["target_" + tag], c["color0"])
        for k, v in b["losses_" + tag].items():
            assert torch.equal(a["losses_" + tag][k], v), (name, tag, k, a["losses_" + tag][k], v)
    for k, g in b["grads"].items():
        assert torch.equal(a["grads"][k], g), (name, k)


def test_single_candidate_form_mutates_the_target_as_upstream():
    from mal_amd import dyn_loss
    c = R.sweep_case("b1_12x35_n1_zero")
    lp = dyn_loss.LossPath(dyn_loss.default_options(height=12, width=35, scales=[0]))
    tgt = dev(c["target"].clone())
    pred = dev(c["cands"][0]).requires_grad_(True)
    cot = torch.rand(1, 1, 12, 35, generator=torch.Generator().manual_seed(5))
    r = lp.compute_reprojection_loss(pred, tgt)
    (r * dev(cot)).sum().backward()
    torch.cuda.synchronize()
    refs = []
    for dt in (F64, F32):
        x = c["cands"][0].to(dt).clone().requires_grad_(True)
        o = R.photo_holes(c["target"], [x], R.F_ZERO_IMG, dt, holes=[R.hole_bytes(c["cands"][0])])
        (o["rp"] * cot.to(dt)).sum().backward()
        refs.append((o, x.grad))
    (o64, g64), (o32, g32) = refs
    assert torch.equal(cpu(tgt), o32["target_after"])
    check(dict(r=cpu(r)), dict(r=o64["rp"].detach()), dict(r=o32["rp"].detach()), forward=True, floor=1e-4)
    ex = R.ssim_exempt_holes(o64, c["target"], c["cands"], R.F_ZERO_IMG).expand(-1, 3, -1, -1)
    check(X.masked(dict(g=cpu(pred.grad)), ex), X.masked(dict(g=g64), ex), X.masked(dict(g=g32), ex), numel=12 * 35, floor=1e-4)
