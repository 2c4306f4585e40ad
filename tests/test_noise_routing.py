"""CPU: which tie-break noise map reaches which pass, on the host side of the DualRefine and four-scale routes.

The automask compares ``min_c r_c <= identity + 1e-5 * noise``: the noise only decides near-tie pixels, so a pass that reads
the wrong map (or none) still passes every free-running parity gate.  Here the library calls are stubbed out and each map is
filled with its own index: every visited (scale, iteration) must receive exactly its map in loop order, and the pose-update
pass ``pose_noise``.  The length checks that keep a short or long list from being silently cut or padded are held too."""
import pytest
import torch

from mal_amd import _lib as L
from mal_amd import dualrefine

B, H, W = 1, 16, 24


def _units(scales, n_losses):
    return [(s, it) for s in scales if s != 1 for it in range(n_losses + 1 if s in (0, 1, 2) else 1)]


def _dicts(scales, n_losses):
    """CPU stand-ins of the dicts loss_step / compute_losses read (values do not matter: nothing is computed)"""
    img = lambda h, w: torch.zeros(B, 3, h, w)
    inputs = {("color", f, 0): img(H, W) for f in (0, -1, 1)}
    inputs[("K", 0)], inputs[("inv_K", 0)] = torch.eye(4).expand(B, 4, 4), torch.eye(4).expand(B, 4, 4)
    T = lambda: torch.eye(4).expand(B, 4, 4).clone()
    outputs = {("cam_T_cam", 0, -1): T(), ("cam_T_cam", 0, 1): T(), ("cam_T_cam", 0, -1, 1): T(),
               "consistency_mask": torch.ones(B, 1, H, W)}
    for s in scales:
        inputs[("color", 0, s)] = img(H >> s, W >> s)
        for it in range(n_losses + 1):
            outputs[("disp", s, it)] = torch.full((B, 1, H >> s, W >> s), 0.5)
            outputs[("depth", 0, s, it)] = torch.ones(B, 1, H, W)
    return inputs, outputs


def _tagged(n):
    return [torch.full((B, 1, H, W), float(i)) for i in range(n)]


def _tag(t):
    return None if t is None else int(t.flatten()[0].item())


CASES = [(scales, nl, pu) for scales in ([0], [0, 2], [0, 1, 2, 3], [2, 3]) for nl in (1, 2) for pu in (False, True)
         if not (pu and 0 not in scales)]


@pytest.mark.parametrize("scales,n_losses,pose_update", CASES,
                         ids=["s%s_n%d_%s" % ("".join(map(str, s)), n, "pu" if p else "nopu") for s, n, p in CASES])
def test_dualrefine_one_call_step_routes_each_noise_map_to_its_unit(monkeypatch, scales, n_losses, pose_update):
    """DualRefineLossPath.loss_step: call c (one per visited scale) receives the maps of its iterations, in loop order; the
    scale-0 call's pose-update pass receives pose_noise"""
    units = _units(scales, n_losses)
    calls = []

    def fake_apply(consts, cfg, *leaves):
        n = cfg[4]
        calls.append(dict(scale=cfg[6], n=n, noises=[_tag(t) for t in consts[6]] if consts[6] is not None else None,
                          pose=None if cfg[9] is None else _tag(cfg[9]["noise"])))
        return (torch.zeros(1), torch.zeros(1) if cfg[9] is not None else None, torch.zeros(4 * L.DR_MAX_ITERS + 4),
                torch.zeros(1, dtype=torch.uint8))

    monkeypatch.setattr(dualrefine.DrLossStepFn, "apply", fake_apply)
    inputs, outputs = _dicts(scales, n_losses)
    lp = dualrefine.DualRefineLossPath(dualrefine.default_options(height=H, width=W, batch_size=B, n_losses=n_losses,
                                                                  scales=scales, disable_pose_updates=not pose_update))
    pose_tag = 100 + len(units)
    lp.loss_step(inputs, outputs, noises=_tagged(len(units)),
                 pose_noise=torch.full((B, 1, H, W), float(pose_tag)) if pose_update else None)
    got = [(c["scale"], it, tag) for c in calls for it, tag in enumerate(c["noises"])]
    assert [(s, it) for s, it, _ in got] == units, (got, units)
    assert [tag for _, _, tag in got] == list(range(len(units))), got
    for c in calls:
        assert c["n"] == len(c["noises"]), c
        assert c["pose"] == (pose_tag if (pose_update and c["scale"] == 0) else None), c


@pytest.mark.parametrize("scales,n_losses", [(s, n) for s in ([0], [0, 2], [0, 1, 2, 3], [2, 3]) for n in (1, 2)],
                         ids=["s%s_n%d" % ("".join(map(str, s)), n) for s in ([0], [0, 2], [0, 1, 2, 3], [2, 3]) for n in (1, 2)])
def test_dualrefine_operator_route_routes_each_noise_map_to_its_unit(monkeypatch, scales, n_losses):
    """DualRefineLossPath.compute_losses: the photometric term AND the consistency weight map of each (scale, iteration)
    read that unit's map, in loop order"""
    from mal_amd import functional as Fn
    from mal_amd import loss_utils
    units = _units(scales, n_losses)
    seen = {"reproj": [], "weight": []}

    def fake_reproj(inputs, outputs, key_tail, cands_keys, ext_mask, noise):
        seen["reproj"].append((key_tail, _tag(noise)))
        return torch.zeros(()), torch.zeros(B, 1, H, W)

    def fake_weight(inputs, outputs, scale, it, ext, rp_map, noise):
        seen["weight"].append(((scale, it), _tag(noise)))
        return torch.ones(B, 1, H, W)

    monkeypatch.setattr(Fn.DistilFn, "apply", lambda *a: (torch.zeros(()), None, torch.zeros(B, 1, H, W)))
    monkeypatch.setattr(loss_utils, "_smooth", lambda disp, color: torch.zeros(()))
    inputs, outputs = _dicts(scales, n_losses)
    lp = dualrefine.DualRefineLossPath(dualrefine.default_options(height=H, width=W, batch_size=B, n_losses=n_losses,
                                                                  scales=scales))
    monkeypatch.setattr(lp, "_reproj_term", fake_reproj)
    monkeypatch.setattr(lp, "_weight_map", fake_weight)
    lp.compute_losses(inputs, outputs, noises=_tagged(len(units)))
    assert seen["reproj"] == [(u, i) for i, u in enumerate(units)], seen["reproj"]
    assert seen["weight"] == [(u, i) for i, u in enumerate(units) if u[1] > 0], seen["weight"]


def test_dualrefine_one_call_step_refuses_a_noise_list_of_the_wrong_length(monkeypatch):
    """one map per visited unit: a shorter or longer list is refused before any call (it used to be cut short, and a unit
    left without a map ran with no tie-break noise at all)"""
    calls = []
    monkeypatch.setattr(dualrefine.DrLossStepFn, "apply", lambda *a: calls.append(a))
    scales, n_losses = [0, 1, 2, 3], 1
    inputs, outputs = _dicts(scales, n_losses)
    lp = dualrefine.DualRefineLossPath(dualrefine.default_options(height=H, width=W, batch_size=B, n_losses=n_losses,
                                                                  scales=scales))
    n = len(_units(scales, n_losses))
    for m in (n - 1, n + 1, 0):
        with pytest.raises(L.MalError):
            lp.loss_step(inputs, outputs, noises=_tagged(m))
    assert not calls


def test_dualrefine_step_function_refuses_an_empty_or_short_noise_list():
    """DrLossStepFn takes None (no maps) or exactly one map per iteration; [] is no longer read as "no maps" """
    leaves = [torch.zeros(B, 1, H, W, requires_grad=True)] * 2 + [torch.eye(4).expand(B, 4, 4).clone()] * 4
    img = torch.zeros(B, 3, H, W)
    for nz in ([], _tagged(1), _tagged(3)):
        consts = (img, img, img, torch.eye(4)[None], torch.eye(4)[None], None, nz, None)
        cfg = (0.1, 100.0, 1e-3, 0, 2, None, 0, None, False, None)
        with pytest.raises(L.MalError, match="one noise map per iteration"):
            dualrefine.DrLossStepFn.apply(consts, cfg, *leaves)


def test_multiscale_step_refuses_a_noise_list_of_the_wrong_length(monkeypatch):
    """loss_step_multiscale / MultiScaleLossFn: exactly one map per scale 0..sclm (a longer list used to be cut short)"""
    from mal_amd import step, trainer
    calls = []
    monkeypatch.setattr(step.MultiScaleLossFn, "apply", lambda *a: calls.append(a))
    sclm = 3
    opt = trainer.default_options(height=H, width=W, batch_size=B, sclm=sclm, distil=False)
    inputs = {("color", f, 0): torch.zeros(B, 3, H, W) for f in (0, -1, 1)}
    for m in (sclm, sclm + 2):
        with pytest.raises(L.MalError, match="one map per scale"):
            step.loss_step_multiscale(opt, inputs, {}, {}, noises=_tagged(m))
    assert not calls
    monkeypatch.undo()
    for m in (0, sclm, sclm + 2):
        with pytest.raises(L.MalError, match="one noise map per scale"):
            step.MultiScaleLossFn.apply(((None,) * 3, [], None, None, None, None, None, _tagged(m)),
                                        (0.1, 100.0, sclm, False, None, False), torch.zeros(1, requires_grad=True))


def test_single_scale_step_refuses_a_noise_map_of_the_wrong_shape():
    from mal_amd import step, trainer
    opt = trainer.default_options(height=H, width=W, batch_size=B)
    inputs = {("color", f, 0): torch.zeros(B, 3, H, W) for f in (0, -1, 1)}
    mono = {(k, 0, f): torch.zeros(B, 1, 3) for k in ("axisangle", "translation") for f in (-1, 1)}
    for shape in ((B, 1, H, W - 1), (B, H, W), (B + 1, 1, H, W), (B, 2, H, W)):
        with pytest.raises(L.MalError, match="tie-break noise must be"):
            step.loss_step(opt, inputs, mono, {}, noise=torch.zeros(shape))
