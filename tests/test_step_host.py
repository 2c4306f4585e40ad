"""CPU: the host side of the three one-call loss steps (mal_amd.step.loss_step / loss_step_multiscale,
DualRefineLossPath.loss_step) with the library calls stubbed out, as tests/test_noise_routing.py does.

What is pinned: the order of draws on the global CPU generator (``config.noise_source``), which option lands in which
positional slot of the ``consts`` / ``cfg`` records handed to the autograd functions, the augmentation-mask normalisation,
and which slot of the loss vectors every key of the returned dicts reads (numbers transcribed from include/mal_hip.h:
244-246 for the 16-float vector, :448-451 for the 48-float one, :496-497,504 for DualRefine's).  Everything is read by
POSITION: the records are tuples (named or not)."""
import pytest
import torch

from mal_amd import _lib as L
from mal_amd import config, dualrefine, step, trainer

B, H, W = 2, 16, 24
SEED = 1234


# ------------------------------------------------------------------------------------------------ stand-ins
def _step_dicts(sclm=0, aug=None, pose4d=True):
    g = torch.Generator().manual_seed(5)
    rnd = lambda *shape: torch.rand(*shape, generator=g)
    inputs = {("color", f, 0): rnd(B, 3, H, W) for f in (0, -1, 1)}
    inputs[("K", 0)], inputs[("inv_K", 0)] = torch.eye(4).expand(B, 4, 4).clone(), torch.eye(4).expand(B, 4, 4).clone()
    mono, outputs = {}, {}
    for s in range(sclm + 1):
        inputs[("color", 0, s)] = inputs[("color", 0, 0)] if s == 0 else rnd(B, 3, H >> s, W >> s)
        mono[("disp", s)], outputs[("disp", s)] = rnd(B, 1, H >> s, W >> s), rnd(B, 1, H >> s, W >> s)
    for k in ("axisangle", "translation"):
        for f in (-1, 1):
            mono[(k, 0, f)] = rnd(B, 2, 1, 3) if pose4d else rnd(B, 1, 3)
    outputs["consistency_mask"] = rnd(B, H, W)
    outputs["lowest_cost"] = rnd(B, H, W)
    outputs["augmentation_mask"] = torch.tensor([0.0, 1.0, 1.0]) if aug is None else aug  # one row more than batch_size
    return inputs, mono, outputs


def _opt(**kw):
    return trainer.default_options(height=H, width=W, batch_size=B, **kw)


def _synth(inputs, outputs, scale):
    return False


class _Rec:
    """recorders of the four autograd functions: each keeps its positional arguments and returns correctly shaped values
    (``arange`` loss vectors; map i of the single-scale step is the constant i, so the name it gets can be read back)"""

    def __init__(self, monkeypatch):
        self.step, self.temporal, self.ms, self.dr = [], [], [], []
        monkeypatch.setattr(step.LossStepFn, "apply", self._step)
        monkeypatch.setattr(step.TemporalLossStepFn, "apply", self._temporal)
        monkeypatch.setattr(step.MultiScaleLossFn, "apply", self._ms)
        monkeypatch.setattr(dualrefine.DrLossStepFn, "apply", self._dr)

    @staticmethod
    def _step_result(cfg):
        n = ((3 if cfg[2] else 4) if cfg[5] else 0) + (1 if cfg[8] is not None and cfg[8][1] else 0) + (2 if cfg[7] else 0)
        return (torch.full((1,), 1000.0), torch.arange(16.0)) + tuple(torch.full((1,), float(i)) for i in range(n))

    def _step(self, *args):
        self.step.append(args)
        return self._step_result(args[7])

    def _temporal(self, *args):
        self.temporal.append(args)
        return self._step_result(args[7])

    def _ms(self, consts, cfg, *leaves):
        self.ms.append((consts, cfg, leaves))
        out = [torch.full((1,), 1000.0), torch.arange(48.0)]
        flags = cfg[8] if len(cfg) > 8 else 0
        if cfg[5] and consts[6] is not None and not (flags & L.STEP_NO_MOTION_MASK):
            out.append(torch.full((B, H, W), 7.0))
        if len(cfg) > 9 and cfg[9]:
            out += [torch.full((1,), float(i)) for i in range(2 * (cfg[2] + 1))]
        return tuple(out)

    def _dr(self, consts, cfg, *leaves):
        c = len(self.dr)
        self.dr.append((consts, cfg, leaves))
        ws = torch.full((1,), c, dtype=torch.uint8)
        return (torch.full((1,), 1000.0), torch.full((1,), 7.0) if cfg[9] is not None else None,
                torch.arange(4.0 * L.DR_MAX_ITERS + 4) + 100 * c, ws)


@pytest.fixture
def rec(monkeypatch):
    return _Rec(monkeypatch)


@pytest.fixture
def noise_source():
    """sets config.noise_source for one test and restores it"""
    prev = config.noise_source

    def set_(v):
        config.noise_source = v
    try:
        yield set_
    finally:
        config.noise_source = prev


def _reference_draws(n):
    """the first n torch.randn((B,1,H,W)) of the seeded global CPU generator, and its state after them"""
    torch.manual_seed(SEED)
    draws = [torch.randn((B, 1, H, W)) for _ in range(n)]
    return draws, torch.get_rng_state()


def _dr_dicts(scales, n_losses):
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
    return inputs, outputs


def _dr_path(scales=(0, 1, 2, 3), n_losses=1, **kw):
    return dualrefine.DualRefineLossPath(dualrefine.default_options(height=H, width=W, batch_size=B, n_losses=n_losses,
                                                                    scales=list(scales), **kw))


# ------------------------------------------------------------------------------------------------ RNG stream
@pytest.mark.parametrize("automask_off", [False, True])
def test_loss_step_cpu_noise_is_one_map_then_one_dead_draw(rec, noise_source, automask_off):
    """loss_utils.py:105-106,178; --disable_automasking does not change it on this route"""
    noise_source("cpu")
    draws, state = _reference_draws(2)
    torch.manual_seed(SEED)
    step.loss_step(_opt(disable_automasking=automask_off), *_step_dicts())
    assert torch.equal(torch.get_rng_state(), state)
    consts, cfg = rec.step[0][6], rec.step[0][7]
    assert torch.equal(consts[8], draws[0]) and cfg[8] is None


def test_multiscale_cpu_noise_is_the_maps_then_as_many_dead_draws(rec, noise_source):
    noise_source("cpu")
    draws, state = _reference_draws(8)
    torch.manual_seed(SEED)
    step.loss_step_multiscale(_opt(sclm=3, distil=False), *_step_dicts(sclm=3))
    assert torch.equal(torch.get_rng_state(), state)
    consts, cfg, _ = rec.ms[0]
    assert len(consts[7]) == 4 and all(torch.equal(a, b) for a, b in zip(consts[7], draws)) and cfg[4] is None


@pytest.mark.parametrize("pose_update", [False, True])
def test_dualrefine_cpu_noise_is_one_map_per_unit_then_the_pose_map(rec, noise_source, pose_update):
    noise_source("cpu")
    n = 6 if pose_update else 5
    draws, state = _reference_draws(n)
    torch.manual_seed(SEED)
    _dr_path().loss_step(*_dr_dicts([0, 1, 2, 3], 1), pose_update=pose_update)
    assert torch.equal(torch.get_rng_state(), state)
    assert [c[1][6] for c in rec.dr] == [0, 2, 3] and [c[1][4] for c in rec.dr] == [2, 2, 1]
    got = [m for c in rec.dr for m in c[0][6]]
    assert len(got) == 5 and all(torch.equal(a, b) for a, b in zip(got, draws))
    assert all(c[1][5] is None for c in rec.dr)
    if pose_update:
        assert torch.equal(rec.dr[0][1][9]["noise"], draws[5])
        assert all(c[1][9] is None for c in rec.dr[1:])
    else:
        assert all(c[1][9] is None for c in rec.dr)


@pytest.mark.parametrize("source", ["cpu", "cuda", "philox"])
def test_disable_automasking_draws_nothing_on_the_multiscale_and_dualrefine_routes(rec, noise_source, source):
    noise_source(source)
    torch.manual_seed(SEED)
    state = torch.get_rng_state()
    step.loss_step_multiscale(_opt(sclm=3, distil=False, disable_automasking=True), *_step_dicts(sclm=3))
    _dr_path(disable_automasking=True).loss_step(*_dr_dicts([0, 1, 2, 3], 1), pose_update=True)
    assert torch.equal(torch.get_rng_state(), state)
    assert rec.ms[0][0][7] is None and rec.ms[0][1][4] is None
    assert all(c[0][6] is None and c[1][5] is None for c in rec.dr)
    assert rec.dr[0][1][9]["noise"] is None


def test_philox_touches_no_generator_and_passes_the_seed(rec, noise_source):
    noise_source("philox")
    torch.manual_seed(SEED)
    state = torch.get_rng_state()
    step.loss_step(_opt(), *_step_dicts())
    step.loss_step(_opt(), *_step_dicts(), want_noise=True)
    step.loss_step_multiscale(_opt(sclm=3, distil=False), *_step_dicts(sclm=3))
    _dr_path().loss_step(*_dr_dicts([0, 1, 2, 3], 1), pose_update=True)
    assert torch.equal(torch.get_rng_state(), state)
    assert rec.step[0][6][8] is None and rec.step[0][7][8] == (config.noise_seed, False)
    assert rec.step[1][6][8] is None and rec.step[1][7][8] == (config.noise_seed, True)
    assert rec.ms[0][0][7] is None and rec.ms[0][1][4] == config.noise_seed
    assert all(c[0][6] is None and c[1][5] == config.noise_seed for c in rec.dr)
    assert rec.dr[0][1][9]["noise"] is None


def test_cuda_noise_makes_no_dead_draws(rec, noise_source, monkeypatch):
    """"cuda": the maps come from ``loss_utils.draw_noise`` (the device generator) and no dead draw follows"""
    from mal_amd import loss_utils
    noise_source("cuda")
    made = []
    monkeypatch.setattr(loss_utils, "draw_noise", lambda shape, dev: made.append(tuple(shape)) or torch.zeros(shape))
    torch.manual_seed(SEED)
    state = torch.get_rng_state()
    step.loss_step(_opt(), *_step_dicts())
    step.loss_step_multiscale(_opt(sclm=3, distil=False), *_step_dicts(sclm=3))
    _dr_path().loss_step(*_dr_dicts([0, 1, 2, 3], 1), pose_update=True)
    assert torch.equal(torch.get_rng_state(), state)
    assert made == [(B, 1, H, W)] * (1 + 4 + 6)


def test_supplied_maps_are_passed_on_and_nothing_is_drawn(rec, noise_source):
    noise_source("cpu")
    torch.manual_seed(SEED)
    state = torch.get_rng_state()
    maps = [torch.full((B, 1, H, W), float(i)) for i in range(6)]
    step.loss_step(_opt(), *_step_dicts(), noise=maps[0])
    step.loss_step_multiscale(_opt(sclm=3, distil=False), *_step_dicts(sclm=3), noises=maps[:4])
    _dr_path().loss_step(*_dr_dicts([0, 1, 2, 3], 1), noises=maps[:5], pose_update=True, pose_noise=maps[5])
    assert torch.equal(torch.get_rng_state(), state)
    assert rec.step[0][6][8] is maps[0]
    assert all(a is b for a, b in zip(rec.ms[0][0][7], maps[:4]))
    assert all(a is b for a, b in zip([m for c in rec.dr for m in c[0][6]], maps[:5]))
    assert rec.dr[0][1][9]["noise"] is maps[5]


# ------------------------------------------------------------------------------------------------ option routing
NZ = torch.zeros(B, 1, H, W)
STEP_DEFAULT = (0.1, 100.0, False, 1.0, 1.0, True, True, False, None, False)
# (min_depth, max_depth, no_ens, w_main, w_distil, want_maps, aug_is_mask, want_decisions, philox, dual_distil)


def _with(row, **at):
    row = list(row)
    for k, v in at.items():
        row[int(k[1:])] = v
    return tuple(row)


@pytest.mark.parametrize("opts,kw,expect", [
    ({}, {}, STEP_DEFAULT),
    ({"no_ens": True}, {}, _with(STEP_DEFAULT, _2=True)),
    ({"dual_distil": True}, {}, _with(STEP_DEFAULT, _9=True)),
    ({"dual_distil": True, "no_ens": True}, {}, _with(STEP_DEFAULT, _2=True, _9=True)),
    ({"loss_blc": True}, {"w_list": [0.3, 0.7], "batch_size_scale": 5}, _with(STEP_DEFAULT, _3=5.0 * 0.3, _4=5.0 * 0.7)),
    ({"loss_blc": True}, {"w_list": [0.3, 0.7]}, _with(STEP_DEFAULT, _3=2.0 * 0.3, _4=2.0 * 0.7)),
    ({}, {"want_maps": False}, _with(STEP_DEFAULT, _5=False)),
    ({}, {"want_decisions": True}, _with(STEP_DEFAULT, _7=True)),
    ({}, {"want_noise": True}, STEP_DEFAULT),  # (read only when the step draws the noise itself)
], ids=["default", "no_ens", "dual_distil", "dual_distil_no_ens", "loss_blc_scale5", "loss_blc_batch_size", "no_maps",
        "decisions", "want_noise_with_a_map"])
def test_loss_step_routes_each_option_to_its_slot(rec, opts, kw, expect):
    inputs, mono, outputs = _step_dicts()
    cmask, lowest = outputs["consistency_mask"], outputs["lowest_cost"]
    step.loss_step(_opt(**opts), inputs, mono, outputs, noise=NZ, **kw)
    assert not rec.temporal and len(rec.step) == 1
    args = rec.step[0]
    assert len(args) == 9 and args[8] is None
    assert tuple(args[7]) == expect
    assert args[0] is mono[("disp", 0)] and args[1] is outputs[("disp", 0)]
    for got, key in zip(args[2:6], (("axisangle", 0, -1), ("translation", 0, -1), ("axisangle", 0, 1), ("translation", 0, 1))):
        assert got.shape == (B, 1, 3) and torch.equal(got, mono[key][:, 0])  # frame 0 of the (B,2,1,3) decoder output
    consts = args[6]
    assert len(consts) == 9
    for got, want in zip(consts[:5], [inputs[("color", f, 0)] for f in (0, -1, 1)] + [inputs[("K", 0)], inputs[("inv_K", 0)]]):
        assert got is want
    assert torch.equal(consts[5], cmask) and consts[7] is lowest and consts[8] is NZ


def test_loss_step_takes_three_dim_poses_as_they_are(rec):
    inputs, mono, outputs = _step_dicts(pose4d=False)
    step.loss_step(_opt(), inputs, mono, outputs, noise=NZ)
    assert all(a is mono[k] for a, k in zip(rec.step[0][2:6], (("axisangle", 0, -1), ("translation", 0, -1),
                                                                ("axisangle", 0, 1), ("translation", 0, 1))))


@pytest.mark.parametrize("flags,which", [({"temporal": True}, (True, False)), ({"main_temporal": True}, (False, True)),
                                         ({"temporal": True, "main_temporal": True}, (True, True))])
def test_loss_step_with_a_hint_calls_the_temporal_function(rec, flags, which):
    inputs, mono, outputs = _step_dicts()
    step.loss_step(_opt(**flags), inputs, mono, outputs, noise=NZ, image_synthesis=_synth)
    assert not rec.step and len(rec.temporal) == 1
    args = rec.temporal[0]
    assert len(args) == 14 and tuple(args[7]) == STEP_DEFAULT
    assert args[8] is _synth and args[9] is inputs and args[10][0] is mono and args[10][1] is outputs
    assert tuple(args[11]) == which and args[12] is None and args[13] is None


def test_loss_step_sclm_hands_the_low_resolution_disparities_teacher_first(rec):
    inputs, mono, outputs = _step_dicts(sclm=2)
    step.loss_step(_opt(sclm=2, temporal=True), inputs, mono, outputs, noise=NZ, image_synthesis=_synth)
    sclm, low_t, low_s = rec.temporal[0][13]
    assert sclm == 2 and len(low_t) == 2 and len(low_s) == 2
    assert all(a is b for a, b in zip((*low_t, *low_s), (mono[("disp", 1)], mono[("disp", 2)], outputs[("disp", 1)],
                                                          outputs[("disp", 2)])))
    # without a hint the other scales are checked but not passed on
    step.loss_step(_opt(sclm=2), inputs, mono, outputs, noise=NZ)
    assert len(rec.step) == 1 and len(rec.step[0]) == 9


def test_loss_step_learn_ens_passes_the_head_as_the_last_leaf(rec):
    inputs, mono, outputs = _step_dicts()
    outputs["ens_disp"] = torch.rand(B, 1, H, W)
    step.loss_step(_opt(learn_ens=True), inputs, mono, outputs, noise=NZ)
    assert rec.step[0][8] is outputs["ens_disp"]
    step.loss_step(_opt(learn_ens=True, temporal=True), inputs, mono, outputs, noise=NZ, image_synthesis=_synth)
    assert rec.temporal[0][12] is outputs["ens_disp"]
    step.loss_step(_opt(learn_ens=True, no_ens=True), inputs, mono, outputs, noise=NZ)
    assert rec.step[1][8] is None


MS_DEFAULT = (0.1, 100.0, 3, True, None, True, None, False, 0, False)
# (min_depth, max_depth, sclm, aug_is_mask, philox, want_maps, hint, no_ssim, extra flags, want_decisions)


@pytest.mark.parametrize("opts,kw,expect", [
    ({}, {}, MS_DEFAULT),
    ({"no_ssim": True}, {}, _with(MS_DEFAULT, _7=True)),
    ({"disable_motion_masking": True}, {"want_maps": False}, _with(MS_DEFAULT, _5=False, _8=L.STEP_NO_MOTION_MASK)),
    ({"no_matching_augmentation": True}, {}, _with(MS_DEFAULT, _8=L.STEP_NO_AUG)),
    ({"ensemble": True}, {}, _with(MS_DEFAULT, _8=L.STEP_ENSEMBLE)),
    ({"disable_motion_masking": True, "no_matching_augmentation": True, "ensemble": True}, {"want_maps": False},
     _with(MS_DEFAULT, _5=False, _8=L.STEP_NO_MOTION_MASK | L.STEP_NO_AUG | L.STEP_ENSEMBLE)),
    ({}, {"want_decisions": True}, _with(MS_DEFAULT, _9=True)),
], ids=["default", "no_ssim", "no_motion_mask", "no_aug", "ensemble", "all_three_bits", "decisions"])
def test_multiscale_routes_each_option_to_its_slot(rec, opts, kw, expect):
    assert (L.STEP_NO_MOTION_MASK, L.STEP_NO_AUG, L.STEP_ENSEMBLE) == (1024, 2048, 4096)  # include/mal_hip.h:286-292
    inputs, mono, outputs = _step_dicts(sclm=3)
    cmask, lowest = outputs["consistency_mask"], outputs["lowest_cost"]
    noises = [NZ.clone() for _ in range(4)]
    res = step.loss_step_multiscale(_opt(sclm=3, distil=False, **opts), inputs, mono, outputs, noises=noises, **kw)
    consts, cfg, leaves = rec.ms[0]
    assert tuple(cfg) == expect
    assert len(consts) == 8
    assert all(a is inputs[("color", f, 0)] for a, f in zip(consts[0], (0, -1, 1))) and len(consts[0]) == 3
    assert len(consts[1]) == 3 and all(a is inputs[("color", 0, s)] for a, s in zip(consts[1], (1, 2, 3)))
    assert consts[2] is inputs[("K", 0)] and consts[3] is inputs[("inv_K", 0)] and torch.equal(consts[4], cmask)
    assert consts[6] is lowest and all(a is b for a, b in zip(consts[7], noises))
    want = [mono[("disp", s)] for s in range(4)] + [outputs[("disp", s)] for s in range(4)]
    assert len(leaves) == 12 and all(a is b for a, b in zip(leaves[:8], want))
    for got, key in zip(leaves[8:], (("axisangle", 0, -1), ("translation", 0, -1), ("axisangle", 0, 1), ("translation", 0, 1))):
        assert torch.equal(got, mono[key][:, 0])
    if kw.get("want_decisions"):
        assert [int(t) for t in res[2]["dec_teacher"]] == [0, 1, 2, 3] and [int(t) for t in res[2]["dec_student"]] == [4, 5, 6, 7]
    else:
        assert len(res) == 2
    if kw.get("want_maps", True):
        assert torch.equal(outputs["consistency_mask"], torch.full((B, H, W), 7.0))  # rewritten with the function's map
    else:
        assert outputs["consistency_mask"] is cmask


def test_multiscale_temporal_hands_the_producer_in_slot_six(rec):
    inputs, mono, outputs = _step_dicts(sclm=1)
    step.loss_step_multiscale(_opt(sclm=1, distil=False, temporal=True), inputs, mono, outputs, noises=[NZ, NZ],
                              image_synthesis=_synth)
    hint = rec.ms[0][1][6]
    assert hint[0] is _synth and hint[1] is inputs and hint[2] is mono


@pytest.mark.parametrize("opts,bit", [({}, 0), ({"disable_automasking": True}, L.DR_NO_AUTOMASK),
                                      ({"disable_motion_masking": True}, L.DR_NO_MOTION_MASK),
                                      ({"avg_reprojection": True}, L.DR_AVG), ({"no_ssim": True}, L.DR_NO_SSIM)],
                         ids=["default", "no_automask", "no_motion_mask", "avg", "no_ssim"])
def test_dualrefine_routes_flags_smoothness_and_texels(rec, opts, bit):
    assert (L.DR_NO_AUTOMASK, L.DR_NO_MOTION_MASK, L.DR_AVG, L.DR_NO_SSIM) == (1, 2, 8, 16)  # include/mal_hip.h:508-511
    inputs, outputs = _dr_dicts([0, 1, 2, 3], 1)
    automask = "disable_automasking" not in opts
    noises = [NZ.clone() for _ in range(5)] if automask else None
    _dr_path(**opts).loss_step(inputs, outputs, noises=noises)
    assert len(rec.dr) == 3
    for c, (consts, cfg, leaves), (scale, n) in zip(range(3), rec.dr, ((0, 2), (2, 2), (3, 1))):
        assert len(cfg) == 10 and len(consts) == 8
        assert tuple(cfg[:2]) == (0.1, 100.0) and cfg[2] == 1e-3 / 2 ** scale and cfg[3] == bit
        assert cfg[4] == n and cfg[5] is None and cfg[6] == scale and cfg[8] is False and cfg[9] is None
        # the first call's workspace (as the function returned it) is where later scales take the texels from
        assert cfg[7] is None if c == 0 else (cfg[7].dtype == torch.uint8 and int(cfg[7]) == 0)
        assert all(a is inputs[k] for a, k in zip(consts[:5], (("color", 0, 0), ("color", -1, 0), ("color", 1, 0), ("K", 0),
                                                                ("inv_K", 0))))
        if n > 1 and "disable_motion_masking" not in opts:
            assert torch.equal(consts[5], outputs["consistency_mask"])
        else:
            assert consts[5] is None
        assert consts[7] is (inputs[("color", 0, scale)] if scale else None)
        assert len(leaves) == 3 * n and all(a is outputs[("disp", scale, it)] for it, a in enumerate(leaves[:n]))


def test_dualrefine_pose_update_pairs_with_the_iterations_own_tensors(rec):
    inputs, outputs = _dr_dicts([0], 1)
    _dr_path(scales=[0]).loss_step(inputs, outputs, noises=[NZ, NZ], pose_update=True, pose_noise=NZ, want_decisions=False)
    consts, cfg, leaves = rec.dr[0]
    assert cfg[9]["into"] == (1, 0, 1, 0) and cfg[9]["noise"] is NZ
    assert len(leaves) == 3 * 2 + 4 and all(t is None for t in leaves[6:])


# ------------------------------------------------------------------------------------------------ augmentation mask
def _aug_cases():
    f32 = torch.tensor([0.0, 1.0, 1.0])
    return {"float32": (f32, True), "float32_4d": (torch.tensor([1.0, 0.0, 1.0]).reshape(3, 1, 1, 1), True),
            "bool": (torch.tensor([False, True, True]), False), "float64": (f32.double(), False),
            "strided_float32": (torch.tensor([0.0, 9.0, 1.0, 9.0, 1.0, 9.0])[::2], False)}


@pytest.mark.parametrize("name", list(_aug_cases()))
@pytest.mark.parametrize("route", ["step", "multiscale"])
def test_augmentation_mask_is_passed_as_itself_or_as_one_minus_mask(rec, name, route):
    mask, as_itself = _aug_cases()[name]
    if route == "step":
        step.loss_step(_opt(), *_step_dicts(aug=mask), noise=NZ)
        keep, flag = rec.step[0][6][6], rec.step[0][7][6]
    else:
        step.loss_step_multiscale(_opt(sclm=1, distil=False), *_step_dicts(sclm=1, aug=mask), noises=[NZ, NZ])
        keep, flag = rec.ms[0][0][5], rec.ms[0][1][3]
    assert flag is as_itself
    assert keep.shape == (B,) and keep.dtype == torch.float32  # only the first opt.batch_size rows
    if as_itself:
        assert keep.data_ptr() == mask.data_ptr() and torch.equal(keep, mask.reshape(-1)[:B])
    else:
        assert torch.equal(keep, 1 - mask.reshape(-1)[:B].to(torch.float32))


# ------------------------------------------------------------------------------------------------ returned dicts
def _slots(d):
    return {k: float(v) for k, v in d.items()}


def test_loss_step_dict_keys_read_their_slots(rec):
    """include/mal_hip.h:244-246"""
    expect = {"reproj_loss/0": 9, "consistency_loss/0": 4, "distil_loss": 6, "loss/0": 10, "loss": 1000, "mono/reproj_loss/0": 0,
              "mono/loss": 2, "smooth_loss/mono": 1, "smooth_loss/multi": 5, "main/reproj_loss/0": 3}
    losses, loss_list, maps = step.loss_step(_opt(), *_step_dicts(), noise=NZ)
    assert _slots(losses) == expect and loss_list is None and losses["loss"].shape == ()
    losses, loss_list, _ = step.loss_step(_opt(loss_blc=True), *_step_dicts(), noise=NZ, w_list=[0.5, 0.5])
    assert _slots(losses) == dict(expect, **{"loss/0": 11}) and [float(t) for t in loss_list] == [11, 6]


@pytest.mark.parametrize("opts,kw,source,expect", [
    ({}, {}, "cpu", {"mono_reproj": 0, "multi_reproj": 1, "consistency_mask": 2, "ens_reproj": 3}),
    ({"no_ens": True}, {}, "cpu", {"mono_reproj": 0, "multi_reproj": 1, "consistency_mask": 2}),
    ({}, {"want_maps": False}, "cpu", {}),
    ({}, {"want_decisions": True}, "cpu", {"mono_reproj": 0, "multi_reproj": 1, "consistency_mask": 2, "ens_reproj": 3,
                                           "dec_teacher": 4, "dec_student": 5}),
    ({}, {"want_maps": False, "want_decisions": True}, "cpu", {"dec_teacher": 0, "dec_student": 1}),
    ({}, {"want_noise": True}, "philox", {"mono_reproj": 0, "multi_reproj": 1, "consistency_mask": 2, "ens_reproj": 3, "noise": 4}),
    ({"no_ens": True}, {"want_noise": True, "want_decisions": True}, "philox",
     {"mono_reproj": 0, "multi_reproj": 1, "consistency_mask": 2, "noise": 3, "dec_teacher": 4, "dec_student": 5}),
    ({}, {"want_noise": True}, "cpu", {"mono_reproj": 0, "multi_reproj": 1, "consistency_mask": 2, "ens_reproj": 3}),
], ids=["default", "no_ens", "no_maps", "decisions", "decisions_only", "philox_noise", "no_ens_noise_decisions",
        "want_noise_but_drawn_on_the_host"])
def test_loss_step_names_the_maps_in_output_order(rec, noise_source, opts, kw, source, expect):
    noise_source(source)
    inputs, mono, outputs = _step_dicts()
    cmask = outputs["consistency_mask"]
    _, _, maps = step.loss_step(_opt(**opts), inputs, mono, outputs, **kw)
    assert {k: int(v) for k, v in maps.items()} == expect and list(maps) == list(expect)
    if kw.get("want_maps", True):
        assert outputs["consistency_mask"] is maps["consistency_mask"]
    else:
        assert outputs["consistency_mask"] is cmask


def test_multiscale_dict_keys_read_their_slots(rec):
    """include/mal_hip.h:448-451: [net][scale][reproj, consistency, smooth, loss], 32 / 33 the totals, 36+s, 40+s, 44+s"""
    expect = {"loss": 1000, "main/loss": 33,
              "reproj_loss/0": 36, "loss/0": 40, "consistency_loss/0": 17, "main/reproj_loss/0": 16, "main/loss/0": 19,
              "smooth_loss/multi/0": 18,
              "reproj_loss/1": 37, "loss/1": 41, "consistency_loss/1": 21, "main/reproj_loss/1": 20, "main/loss/1": 23,
              "smooth_loss/multi/1": 22,
              "reproj_loss/2": 38, "loss/2": 42, "consistency_loss/2": 25, "main/reproj_loss/2": 24, "main/loss/2": 27,
              "smooth_loss/multi/2": 26,
              "reproj_loss/3": 39, "loss/3": 43, "consistency_loss/3": 29, "main/reproj_loss/3": 28, "main/loss/3": 31,
              "smooth_loss/multi/3": 30}
    mono_expect = {"loss": 32,
                   "smooth_loss/0": 2, "reproj_loss/0": 0, "loss/0": 3, "smooth_loss/1": 6, "reproj_loss/1": 4, "loss/1": 7,
                   "smooth_loss/2": 10, "reproj_loss/2": 8, "loss/2": 11, "smooth_loss/3": 14, "reproj_loss/3": 12, "loss/3": 15}
    noises = [NZ] * 4
    losses, mono_losses = step.loss_step_multiscale(_opt(sclm=3, distil=False), *_step_dicts(sclm=3), noises=noises)
    assert _slots(losses) == expect and _slots(mono_losses) == mono_expect and losses["loss"].shape == ()
    losses, mono_losses = step.loss_step_multiscale(_opt(sclm=3, distil=False, ensemble=True), *_step_dicts(sclm=3), noises=noises)
    ens = {"ensemble_loss/0": 44, "ensemble_loss/1": 45, "ensemble_loss/2": 46, "ensemble_loss/3": 47}
    assert _slots(losses) == dict(expect, **ens) and _slots(mono_losses) == mono_expect
    losses, mono_losses = step.loss_step_multiscale(_opt(sclm=1, distil=False), *_step_dicts(sclm=1), noises=noises[:2])
    assert _slots(losses) == {k: v for k, v in expect.items() if k[-1] not in "23"}
    assert _slots(mono_losses) == {k: v for k, v in mono_expect.items() if k[-1] not in "23"}


def test_dualrefine_dict_keys_read_their_slots(rec):
    """include/mal_hip.h:496-497 with MAL_DR_MAX_ITERS = 4: [4*it + 1] the consistency term, [4*(n-1)] the last iteration's
    reprojection term, [17] the final running loss; call c of the step returns arange + 100*c and a total of 1000"""
    assert L.DR_MAX_ITERS == 4
    expect = {"reproj_loss/0": 4, "loss/0_0": 17, "loss/0_1": 17, "consistency_loss/0_1": 5,
              "reproj_loss/2": 104, "loss/2_0": 117, "loss/2_1": 117, "consistency_loss/2_1": 105,
              "reproj_loss/3": 200, "loss/3_0": 217, "loss": 3000 / 4}
    noises = [NZ] * 5
    losses = _dr_path().loss_step(*_dr_dicts([0, 1, 2, 3], 1), noises=noises, pose_update=False)
    assert _slots(losses) == expect
    rec.dr.clear()
    losses = _dr_path().loss_step(*_dr_dicts([0, 1, 2, 3], 1), noises=noises, pose_update=True, pose_noise=NZ)
    assert _slots(losses) == dict(expect, **{"reproj_loss/pose_0": 7, "loss/pose_0_0": 7, "loss": 3000 / 4 + 7})
    assert losses["reproj_loss/pose_0"] is losses["loss/pose_0_0"]
    rec.dr.clear()
    losses = _dr_path(scales=[0], n_losses=2).loss_step(*_dr_dicts([0], 2), noises=noises[:3], pose_update=False)
    assert _slots(losses) == {"reproj_loss/0": 8, "loss/0_0": 17, "loss/0_1": 17, "loss/0_2": 17, "consistency_loss/0_1": 5,
                              "consistency_loss/0_2": 9, "loss": 1000}


# ------------------------------------------------------------------------------------------------ the records
RECORDS = {
    "StepConsts": (step, ["color0", "color_m1", "color_p1", "K", "inv_K", "cmask", "keep", "lowest", "noise"], 9, 9),
    "StepCfg": (step, ["min_depth", "max_depth", "no_ens", "w_main", "w_distil", "want_maps", "aug_is_mask", "want_decisions",
                       "philox", "dual_distil"], 9, 10),
    "MsConsts": (step, ["colors", "colors_s", "K", "inv_K", "cmask", "keep", "lowest", "noises"], 8, 8),
    "MsCfg": (step, ["min_depth", "max_depth", "sclm", "aug_is_mask", "philox", "want_maps", "hint", "no_ssim", "extra_flags",
                     "want_decisions"], 6, 10),
    "DrConsts": (dualrefine, ["color0", "color_m1", "color_p1", "K", "inv_K", "cmask", "noises", "color0_s"], 7, 8),
    "DrCfg": (dualrefine, ["min_depth", "max_depth", "smooth_weight", "flags", "n", "philox", "scale", "texels_from",
                           "want_decisions", "pose_update"], 6, 10),
}


@pytest.mark.parametrize("name", list(RECORDS))
def test_records_keep_the_positional_order_and_take_the_short_and_the_long_tuple(name):
    module, fields, shortest, longest = RECORDS[name]
    if not hasattr(module, name):
        pytest.skip("the tree has no named records")
    rec_t = getattr(module, name)
    assert list(rec_t._fields) == fields and issubclass(rec_t, tuple)
    for n in (shortest, longest):
        plain = tuple(object() for _ in range(n))
        r = rec_t(*plain)
        assert tuple(r)[:n] == plain and len(r) == len(fields)
    defaults = {"dual_distil": False, "hint": None, "no_ssim": False, "extra_flags": 0, "want_decisions": False, "scale": 0,
                "texels_from": None, "pose_update": None, "color0_s": None}
    r = rec_t(*range(shortest))
    assert {f: getattr(r, f) for f in fields[shortest:]} == {f: defaults[f] for f in fields[shortest:]}
