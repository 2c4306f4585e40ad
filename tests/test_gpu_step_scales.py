"""GPU: --distil with --scales 0 1 2 3 (sclm = 3) in the one-call step (mal_amd.step.loss_step): the extra scales' warps
(mal_loss_step_warp_scales) go to the temporal hint's producer after scale 0 in upstream's order, the LAST call's answer
decides whether scale 0's synthesised candidates join the min, and nothing of the lower scales reaches a loss
(manydepth/trainer.py:1088-1165, loss_utils.py:57-200)."""
import numpy as np
import pytest
import torch

from mal_amd.synthetic import fake_image_synthesis
from oracle import mal_oracle as O
from tests import golden_io as G
from tests import hip_harness as HH
from tests.test_step_scales import SCALE_CASES, producer_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCLM = 3


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


def lowres_of(batch, z=None):
    """the lower scales' disparities: the fixture's (fp16-rounded pooled maps) or pooled copies of scale 0 (HH._lowres)"""
    out = {}
    for name in ("disp_teacher", "disp_student"):
        out[name] = {s: (torch.from_numpy(z["in/%s_s%d" % (name, s)].astype(np.float32)) if z is not None
                         else HH._lowres(batch, name, s)) for s in range(1, SCLM + 1)}
    return out


def add_scales(low, mono_outputs, outputs, leaves, device, dtype=torch.float32, requires_grad=True):
    for s in range(1, SCLM + 1):
        for name, outs in (("disp_teacher", mono_outputs), ("disp_student", outputs)):
            if s not in low[name]:
                continue
            leaf = low[name][s].to(dtype).to(device).clone().requires_grad_(requires_grad)
            leaves["%s_s%d" % (name, s)] = leaf
            outs[("disp", s)] = leaf


def run_step(b, kw, n0, low, producer, want_maps=True):
    """the one-call step on the device with ("disp", s) of both networks for s <= kw["sclm"]"""
    from mal_amd import step, trainer
    from mal_amd.synthetic import to_dicts
    B, _, H, W = b["color0"].shape
    dev = torch.device(DEV)
    opt = trainer.default_options(height=H, width=W, batch_size=B, **kw)
    inputs, mono_outputs, outputs, leaves = to_dicts(b, lambda a, t, inv: None, device=dev)
    if kw.get("sclm"):
        add_scales(low, mono_outputs, outputs, leaves, dev)
    for f, s in ((-1, "m1"), (1, "p1")):
        mono_outputs[("axisangle", 0, f)] = leaves["axisangle_" + s]
        mono_outputs[("translation", 0, f)] = leaves["translation_" + s]
    losses, _, maps = step.loss_step(opt, inputs, mono_outputs, outputs, w_list=[0.7, 0.3], noise=n0.to(dev), want_maps=want_maps,
                                     image_synthesis=producer)
    losses["loss"].backward()
    torch.cuda.synchronize()
    return dict(losses={k: float(v.detach()) for k, v in losses.items()}, leaves=leaves, mono_outputs=mono_outputs,
                outputs=outputs, grads={k: t.grad for k, t in leaves.items()})


def run_oracle_scales(b, kw, n0, n1, low, producer):
    """the free-running CPU oracle with ("disp", s) for s <= sclm: the per-scale warps and samples it leaves"""
    from mal_amd.synthetic import to_dicts
    B, _, H, W = b["color0"].shape
    opt = O.default_opt(height=H, width=W, batch_size=B, **kw)
    inputs, mono_outputs, outputs, leaves = to_dicts(b, O.transformation_from_parameters)
    add_scales(low, mono_outputs, outputs, leaves, "cpu")
    losses, _, _, _, _ = O.mal_loss_step(opt, inputs, mono_outputs, outputs, n0.clone(), n1.clone(), [0.7, 0.3], synth=producer)
    return losses, mono_outputs, outputs


def four_scale_dicts(monkeypatch, low, producer=None):
    """make the shared drivers (tests/hip_harness.py, tests/test_gpu_decisions.py) build sclm = 3 dicts: every to_dicts call
    also adds ("disp", s) leaves; ``producer(batch, device)`` replaces HH.producer_of"""
    import mal_amd.synthetic as S
    orig = S.to_dicts

    def to_dicts(batch, pose_fn, device=None, requires_grad=True):
        inputs, mono_outputs, outputs, leaves = orig(batch, pose_fn, device=device, requires_grad=requires_grad)
        add_scales(low, mono_outputs, outputs, leaves, device or "cpu", batch["disp_teacher"].dtype, requires_grad)
        return inputs, mono_outputs, outputs, leaves

    monkeypatch.setattr(S, "to_dicts", to_dicts)
    monkeypatch.setattr(HH, "to_dicts", to_dicts)
    if producer is not None:
        monkeypatch.setattr(HH, "producer_of", producer)


def fixture_producer(z, b):
    """HH.producer_of for a fixture.  ``lastnone``: the shared drivers list the teacher's candidates by the presence of
    ("syn", f, 0) in the pass's dict; where the last call reports no instance upstream never reads them, so the call at the
    last scale also drops them from that dict (the step's producer sees a per-scale dict: nothing to drop there)"""
    synth = producer_of(z, b)
    if str(z["producer"]) != "lastnone":
        return lambda batch, device=None: synth

    def last_drops(inputs, outputs, scale):
        if scale == int(z["sclm"]):
            outputs.pop(("syn", -1, 0), None)
            outputs.pop(("syn", 1, 0), None)
        return synth(inputs, outputs, scale)

    return lambda batch, device=None: last_drops


def hold_warps(h_outs, o_outs, H, W, s, tol=1e-5):
    """("color", f, s) of the step against the oracle's at 1e-5, except where a sampling position is within rounding of a
    tap switch or the border clip (HH.sample_ambiguous)"""
    amb = HH.sample_ambiguous({f: o_outs[("sample", f, s)].detach().numpy() for f in (-1, 1)}, H, W)
    for f in (-1, 1):
        d = np.abs(h_outs[("color", f, s)].detach().cpu().numpy() - o_outs[("color", f, s)].detach().numpy())
        bad = (d > tol) & ~amb
        assert not bad.any(), (f, s, float(d.max()), int(bad.sum()))
    return amb


@pytest.mark.parametrize("tag", SCALE_CASES)
def test_fixtures_at_golden_size(tag, monkeypatch):
    """each reference fixture: decision-exact against the (forced) oracle under the project's gates -- the oracle
    reproduces the fixture bit for bit (tests/test_step_scales.py) --, the losses against the fixture at the step
    tolerance, the lower scales' warps at 1e-5 (the producer's syn is its output on exactly those warps) and no gradient
    for ("disp", s > 0)"""
    from tests.test_gpu_decisions import check_step_decision_exact
    z = G.load(tag)
    b = G.batch_from_golden(z)
    B, _, H, W = b["color0"].shape
    kw = G.opt_kwargs(z)
    n0, n1 = G.noises(z, (B, 1, H, W))
    low = lowres_of(b, z)
    with monkeypatch.context() as m:
        four_scale_dicts(m, low, fixture_producer(z, b))
        (h, o), _, _ = check_step_decision_exact(b, kw, n0, n1, return_runs=True)
    assert abs(h["losses"]["loss"] - float(z["final_loss"])) <= 1e-4 * abs(float(z["final_loss"]))
    r = run_step(b, kw, n0, low, producer_of(z, b))
    assert r["losses"] == h["losses"]  # (the instrumented run takes the same arithmetic)
    for k in ("reproj_loss/0", "consistency_loss/0", "distil_loss", "loss"):
        assert abs(r["losses"][k] - float(z["losses/" + k])) <= 1e-4 * abs(float(z["losses/" + k])) + 1e-7, k
    for k, t in r["leaves"].items():
        if k[-3:] in ("_s1", "_s2", "_s3"):
            assert t.grad is None, k
    _, mo, oo = run_oracle_scales(b, kw, n0, n1, low, producer_of(z, b))
    synth = producer_of(z, b)
    for who, hd, od, on in (("mono", r["mono_outputs"], mo, kw.get("temporal")), ("multi", r["outputs"], oo, kw.get("main_temporal"))):
        if not on:
            continue
        for s in range(1, SCLM + 1):
            hold_warps(hd, od, H, W, s)
            want = {("color", f, s): hd[("color", f, s)].detach().cpu() for f in (-1, 1)}
            has = synth(None, want, s)
            assert has == (("syn", -1, s) in hd)
            if has:
                for f in (-1, 1):
                    assert torch.equal(hd[("syn", f, s)].detach().cpu(), want[("syn", f, s)]), (who, f, s)
    assert r["mono_outputs"]["has_ins"] == bool(int(z["has_ins"]))


def _batch(tag="step_b2_48x96_sclm3_temporal"):
    z = G.load(tag)
    b = G.batch_from_golden(z)
    B, _, H, W = b["color0"].shape
    n0, _ = G.noises(z, (B, 1, H, W))
    return z, b, n0, lowres_of(b, z)


def _assert_bitwise(a, c):
    assert a["losses"] == c["losses"]
    for k in HH.LEAVES:
        assert torch.equal(a["grads"][k], c["grads"][k]), k


def test_the_last_call_decides():
    """producer answers True, True, True, False: the scale-0 synthesised candidates drop out of the min -- bitwise the
    sclm = 0 step whose producer finds nothing (trainer.py:1162: has_ins is overwritten per scale)"""
    z, b, n0, low = _batch()
    synth = fake_image_synthesis(b["syn_rects"])
    tttf = lambda inputs, outputs, scale: False if scale == SCLM else synth(inputs, outputs, scale)
    a = run_step(b, {"temporal": True, "sclm": SCLM}, n0, low, tttf)
    c = run_step(b, {"temporal": True}, n0, low, lambda i, o, s: False)
    _assert_bitwise(a, c)
    assert a["mono_outputs"]["has_ins"] is False and ("syn", -1, 0) not in a["mono_outputs"]
    assert ("syn", -1, 1) in a["mono_outputs"] and ("syn", -1, SCLM) not in a["mono_outputs"]


def test_upstreams_key_error_and_a_clean_next_step():
    """scale 0 reports nothing, scale 3 reports instances: upstream's compute_losses reads ("syn", -1, 0), which was never
    written -- KeyError.  The step is abandoned (mal_loss_step_abort) and the next one on the same workspace runs as before"""
    z, b, n0, low = _batch()
    synth = fake_image_synthesis(b["syn_rects"])
    kw = {"temporal": True, "sclm": SCLM}
    ref = run_step(b, kw, n0, low, synth)
    late = lambda inputs, outputs, scale: False if scale == 0 else synth(inputs, outputs, scale)
    with pytest.raises(KeyError) as e:
        run_step(b, kw, n0, low, late)
    assert e.value.args[0] == ("syn", -1, 0)
    again = run_step(b, kw, n0, low, synth)
    _assert_bitwise(again, ref)


def test_the_producer_sees_every_scale_in_upstreams_order():
    """--temporal --main_temporal: teacher scales 0..3, then student scales 0..3, each a (B,3,H,W) full-resolution warp
    equal to the oracle's for that pass and scale"""
    z, b, n0, low = _batch("step_b2_48x96_sclm3_temporal_main")
    B, _, H, W = b["color0"].shape
    synth = fake_image_synthesis(b["syn_rects"])
    seen = []

    def spy(inputs, outputs, scale):
        seen.append((scale, {f: outputs[("color", f, scale)].detach().cpu().clone() for f in (-1, 1)}))
        return synth(inputs, outputs, scale)

    kw = {"temporal": True, "main_temporal": True, "sclm": SCLM}
    run_step(b, kw, n0, low, spy)
    assert [s for s, _ in seen] == [0, 1, 2, 3, 0, 1, 2, 3]
    _, mo, oo = run_oracle_scales(b, kw, n0, n0, low, synth)
    for i, (s, warps) in enumerate(seen):
        od = mo if i < 4 else oo
        for f in (-1, 1):
            assert tuple(warps[f].shape) == (B, 3, H, W)
        hold_warps({("color", f, s): warps[f] for f in (-1, 1)}, od, H, W, s)


def test_without_a_hint_the_lower_scales_change_nothing():
    """sclm = 3 without --temporal: no extra device work, every loss and every gradient bitwise the sclm = 0 step's, and
    the lower scales' disparities receive no gradient"""
    z, b, n0, low = _batch()
    a = run_step(b, {"sclm": SCLM}, n0, low, None)
    c = run_step(b, {}, n0, low, None)
    _assert_bitwise(a, c)
    for k, t in a["leaves"].items():
        if k[-3:] in ("_s1", "_s2", "_s3"):
            assert t.grad is None, k


def test_loss_step_refuses_what_it_does_not_cover():
    from mal_amd import _lib as L
    z, b, n0, low = _batch()
    synth = fake_image_synthesis(b["syn_rects"])
    for kw in ({"sclm": 4}, {"sclm": SCLM, "v1_multiscale": True}, {"sclm": SCLM, "frame_ids": [0, 1, -1]},
               {"sclm": SCLM, "no_ssim": True}):
        with pytest.raises(L.MalError):
            run_step(b, dict(kw, temporal=True), n0, low, synth)
    bad = {k: dict(v) for k, v in low.items()}
    bad["disp_student"][2] = bad["disp_student"][2][..., :-1]
    with pytest.raises(L.MalError):
        run_step(b, {"sclm": SCLM, "temporal": True}, n0, bad, synth)
    cut = {k: dict(v) for k, v in low.items()}
    del cut["disp_teacher"][3]
    with pytest.raises(KeyError):  # as upstream: generate_images_pred reads ("disp", 3)
        run_step(b, {"sclm": SCLM, "temporal": True}, n0, cut, synth)


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
def test_operator_route_agrees(fuse, monkeypatch):
    """MALLossPath.compute_batch_losses with sclm = 3 --distil --temporal (its own per-scale loop, trainer.py:1088-1165) and
    the one-call step: the same numbers at the gates of tests/test_gpu_step.py::test_loss_step_equals_operator_route"""
    z, b, n0, low = _batch()
    B, _, H, W = b["color0"].shape
    _, n1 = G.noises(z, (B, 1, H, W))
    kw = {"temporal": True, "sclm": SCLM}
    a = run_step(b, kw, n0, low, fake_image_synthesis(b["syn_rects"]))
    with monkeypatch.context() as m:
        four_scale_dicts(m, low)
        c = HH.run_hip(b, kw, n0, n1, fuse=fuse)
    assert abs(a["losses"]["loss"] - c["final"]) <= 2e-6 * abs(c["final"]), (a["losses"]["loss"], c["final"])
    for k in HH.LEAVES:
        ga, gc = a["grads"][k].cpu().numpy(), c["grads"][k]
        assert np.abs(ga - gc).max() <= 2e-5 * np.abs(gc).max(), (k, np.abs(ga - gc).max() / np.abs(gc).max())


def _headline_batch():
    from mal_amd.synthetic import make_batch
    B, H, W = 12, 192, 640
    b = make_batch(B, H, W, seed=1234)
    b["syn_instances"] = (3, 1234)  # bench.py: instance_stub(B, H, W, n_inst=3, seed=1234 + rank)
    return b


def test_headline_with_four_scales_decision_exact(monkeypatch):
    """BASELINE configs[1] as named -- B=12 192x640, --temporal --distil, four scales -- with the real producer
    (mal_amd.dyn_utils.image_synthesis, stand-in segmenter, three instances) against the CPU oracle running the same
    four-scale loop with the restated producer: decision-exact under the README's gradient gate
    (tests/test_gpu_decisions.py::check_step_decision_exact).  The lower scales are pooled copies (HH._lowres)."""
    from tests.test_gpu_decisions import check_step_decision_exact
    b = _headline_batch()
    B, _, H, W = b["color0"].shape
    g = torch.Generator().manual_seed(8)
    n0, n1 = torch.randn(B, 1, H, W, generator=g), torch.randn(B, 1, H, W, generator=g)
    with monkeypatch.context() as m:
        four_scale_dicts(m, lowres_of(b))
        (h, o), counts, report = check_step_decision_exact(b, {"temporal": True, "sclm": SCLM}, n0, n1, return_runs=True)
    won = HH.kernel_decisions(h["maps"])["teacher"]["win"] >= 2
    assert 0.001 < float(won.float().mean()) < 0.2, float(won.float().mean())
    print("headline with four scales: differing decisions", counts, "L2 rel to fp64 (hip, fp32 oracle)", report)


def test_headline_with_four_scales_replays_from_a_graph():
    """the same step captured into one HIP graph (as bench.py replays the headline): a replay leaves the eager run's loss and
    gradients bit for bit, the lower scales' warps included"""
    from mal_amd import step, trainer
    from mal_amd.synthetic import to_dicts
    b = _headline_batch()
    B, _, H, W = b["color0"].shape
    dev = torch.device(DEV)
    n0 = torch.randn(B, 1, H, W, generator=torch.Generator().manual_seed(9)).to(dev)
    opt = trainer.default_options(height=H, width=W, batch_size=B, temporal=True, sclm=SCLM)
    inputs, mono_outputs, outputs, leaves = to_dicts(b, lambda a, t, inv: None, device=dev)
    add_scales(lowres_of(b), mono_outputs, outputs, leaves, dev)
    for f, sfx in ((-1, "m1"), (1, "p1")):
        mono_outputs[("axisangle", 0, f)] = leaves["axisangle_" + sfx]
        mono_outputs[("translation", 0, f)] = leaves["translation_" + sfx]
    synth = HH.producer_of(b, dev)
    one_ = torch.ones((), device=dev)
    hold = {}

    def one():
        for t in leaves.values():
            t.grad = None
        mo = dict(mono_outputs)
        losses, _, _ = step.loss_step(opt, inputs, mo, dict(outputs), w_list=[0.7, 0.3], noise=n0, want_maps=False,
                                      image_synthesis=synth)
        losses["loss"].backward(gradient=one_)
        hold["loss"] = losses["loss"].detach()
        hold["warp"] = mo[("color", -1, SCLM)]

    s_ = torch.cuda.Stream()  # eager steps on a side stream, as tests/test_gpu_step.py and bench.py capture
    s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        one()
        one()
    torch.cuda.current_stream().wait_stream(s_)
    torch.cuda.synchronize()
    ref_loss = float(hold["loss"])
    ref = {k: t.grad.clone() for k, t in leaves.items() if t.grad is not None}
    ref_warp = hold["warp"].clone()
    assert set(ref) == set(HH.LEAVES)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        one()
    grads = {k: t.grad for k, t in leaves.items() if k in ref}
    warp = hold["warp"]
    for _ in range(2):
        for t in grads.values():
            t.zero_()
        warp.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert float(hold["loss"]) == ref_loss
        for k, t in grads.items():
            assert torch.equal(t, ref[k]), k
        assert torch.equal(warp, ref_warp)
