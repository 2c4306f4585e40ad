"""The task decomposition and the process-wide scheduling options (mal_set_option) are scheduling choices only.

Every marching kernel splits an image into 60/62-column strips and each strip into row segments whose height is picked from
the device's CU count; window sums are formed "outer rows first", boundary rows are handed over through scratch rows and
per-task partials are reduced in a fixed order, so that the per-pixel decisions do not depend on where the segment
boundaries fall.  Here the decomposition is swept ("march_rows", "march_rows_fwd", "pack_rows", "syn_rows", "march_halo1" x
"march_flip", "device_cus": the decompositions a CPX partition, an MI300X or a larger part would pick) at ragged shapes for
the one-call step (--distil, --temporal, --temporal --main_temporal), the four-scale step and DualRefine's step:
  (i)   the exported decision planes are bitwise the default decomposition's,
  (ii)  the loss scalars are within 1e-6 rel of the default's, the gradients within 1e-5 (sums in another order),
  (iii) one non-default decomposition per step and shape runs the existing decision-exact checks against the forced oracle
        with their gates unchanged.
The overlap switches must leave losses and gradients bitwise unchanged, eagerly and replayed from a graph; the N4
VJPs hold their fixtures under every "epi_bwd_planes"; and a step whose decomposition options change between its forward
and its backward is refused (MAL_ESTALE) instead of assembling gradients from the wrong segments.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import golden_io as G
from tests import hip_harness as HH

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

# every name mal_set_option accepts is either swept here (the values used) or excluded with a reason;
# tests/test_options.py holds this list to the library's source and header
SWEPT = {
    "march_rows": "8, 9, 13, H-1, H, 4096",
    "march_rows_fwd": "8, 11, 4096",
    "pack_rows": "8, 9, 17, 4096",
    "syn_rows": "2, 3, 7, 8, 64",
    "march_halo1": "0, 1 (x march_flip)",
    "march_flip": "0, 1 (x march_halo1)",
    "device_cus": "1, 32, 80, 304, 1024",
    "step_overlap": "0, 2",
    "student_overlap": "0",
    "side_order": "1",
    "side_priority": "1 (fresh process)",
    "sweeps_batched": "0",
    "ms_fold": "0",
    "epi_bwd_planes": "0, 1",
}
EXCLUDED = {
    "debug": "a probe: instruments kernels for timing experiments, results not meant to be used",
    "epi_probe": "a probe: timing experiments of the plane kernel that give wrong results by design",
    "pass_impl": "experiments-only formulations (0 / 2): the default build refuses them (tests/test_gpu_layers.py)",
    "temporal_spec": "experiments-only: the default build refuses 1 (tests/test_gpu_step.py covers the experiments build)",
    "march3": "experiments-only: the default build refuses 1 (tests/test_gpu_step.py covers the experiments build)",
    "syn_queue": "experiments-only: the default build refuses 1",
    "march_lean": "held bit for bit against the generic instantiations in tests/test_gpu_step.py",
    "tail_overlap": "held against the serial backward, eager and graph, in tests/test_gpu_step.py",
    "photo_impl": "a different summation order by design (ATen's); both held against the oracle in tests/test_gpu_layers.py",
    "costvol_impl": "both formulations held in tests/test_gpu_costvol.py and tests/test_gpu_costvol_sweep.py",
    "dyn_small_blocks": "held in tests/test_gpu_dyn.py",
}


def _lib():
    from mal_amd import _lib as L
    return L.load()


def get_option(name):
    v = ctypes.c_int()
    assert _lib().mal_get_option(name.encode(), ctypes.byref(v)) == 0, name
    return v.value


def set_options(**kw):
    from mal_amd import _lib as L
    for k, v in kw.items():
        L.check(_lib().mal_set_option(k.encode(), int(v)), "mal_set_option(%s, %d)" % (k, v))


ALL_NAMES = sorted(set(SWEPT) | set(EXCLUDED))


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


@pytest.fixture(autouse=True)
def _restore_options():
    """every option as it was before the test, failures included"""
    saved = {k: get_option(k) for k in ALL_NAMES}
    try:
        yield
    finally:
        for k, v in saved.items():
            _lib().mal_set_option(k.encode(), v)


def _grads_close(g, r):
    """disparity maps: every pixel within 1e-5 of the map's scale; pose vectors (sums of many cancelling per-task partials,
    reduced in another order): 1e-5 L2 rel"""
    assert set(g) == set(r)
    for k in r:
        if np.ndim(r[k]) == 4:
            sc = max(float(np.abs(r[k]).max()), 1e-30)
            err = float(np.abs(g[k] - r[k]).max()) / sc
        else:
            err = float(np.linalg.norm((g[k] - r[k]).ravel()) / (np.linalg.norm(np.ravel(r[k])) + 1e-30))
        assert err <= 1e-5, (k, "distance from the default decomposition's gradient", err)


def _losses_close(l, r, tol=1e-6):
    assert set(l) == set(r)
    for k, v in r.items():
        if v is None:
            continue
        assert abs(l[k] - v) <= tol * abs(v) + 1e-12, (k, l[k], v)


# ---- the one-call step: --distil, --temporal, --temporal --main_temporal

STEP_KINDS = {"distil": {}, "temporal": {"temporal": True}, "both": {"temporal": True, "main_temporal": True}}
SHAPES = [(2, 40, 130), (3, 37, 50), (1, 16, 61), (2, 10, 121)]


def decomposition_configs(H):
    """the sweep, options combined where they interact (march_rows x march_flip x march_halo1, the forward's rows against the
    gradient passes', the packing sweep's and the fused sweep's rows against both)"""
    return [
        {"march_rows": 8}, {"march_rows": 9, "march_flip": 0}, {"march_rows": 13, "march_halo1": 0},
        {"march_rows": max(H - 1, 8), "march_rows_fwd": 11}, {"march_rows": H, "march_flip": 0, "march_halo1": 0},
        {"march_rows": 4096, "pack_rows": 4096},
        {"march_rows_fwd": 8, "pack_rows": 9}, {"march_rows_fwd": 4096, "march_rows": 9, "syn_rows": 7},
        {"pack_rows": 8, "syn_rows": 2}, {"pack_rows": 17, "syn_rows": 3}, {"syn_rows": 8}, {"syn_rows": 64, "march_rows": 13},
        {"march_halo1": 0, "march_flip": 1}, {"march_halo1": 1, "march_flip": 0}, {"march_halo1": 0, "march_flip": 0},
        {"device_cus": 1}, {"device_cus": 32, "march_flip": 0}, {"device_cus": 80}, {"device_cus": 304, "march_halo1": 0},
        {"device_cus": 1024},
    ]


def _step_run(b, kw, n0):
    from tests.test_gpu_decisions import run_step_with_decisions
    h = run_step_with_decisions(b, kw, n0)
    return h["losses"], {k: h["maps"][k] for k in ("dec_teacher", "dec_student")}, h["grads"]


def _hold_like_default(run, ref, cfg):
    l, d, g = run
    l0, d0, g0 = ref
    for k in d0:
        same = torch.equal(d[k], d0[k])
        assert same, (cfg, k, "decision plane differs from the default decomposition's at",
                      int((d[k] != d0[k]).sum()), "entries")
    _losses_close(l, l0)
    _grads_close(g, g0)


@pytest.mark.parametrize("B,H,W", SHAPES, ids=["b2_40x130", "b3_37x50", "b1_16x61", "b2_10x121"])
@pytest.mark.parametrize("kind", list(STEP_KINDS))
def test_step_decomposition_sweep(kind, B, H, W):
    from mal_amd.synthetic import make_batch
    from tests.test_gpu_decisions import check_step_decision_exact
    kw = STEP_KINDS[kind]
    b = make_batch(B, H, W, seed=57, with_syn=bool(kw))
    g = torch.Generator().manual_seed(11)
    n0, n1 = torch.randn(B, 1, H, W, generator=g), torch.randn(B, 1, H, W, generator=g)
    ref = _step_run(b, kw, n0)
    for cfg in decomposition_configs(H):
        set_options(march_rows=0, march_rows_fwd=0, pack_rows=10, syn_rows=4, march_halo1=1, march_flip=1, device_cus=0)
        set_options(**cfg)
        _hold_like_default(_step_run(b, kw, n0), ref, cfg)
    if (B, H, W) in SHAPES[:2]:
        # a non-default decomposition through the decision-exact check against the forced oracle, gates unchanged
        set_options(march_rows=9, march_rows_fwd=11, pack_rows=17, syn_rows=3, march_halo1=1, march_flip=0, device_cus=0)
        counts, report = check_step_decision_exact(b, kw, n0, n1)
        assert all(v[0] <= 1e-4 for v in report.values()), report


# ---- the four-scale step

def _ms_run(batch, kw, nt, matching=True):
    from mal_amd import step, trainer
    sclm = kw["sclm"]
    hi, hm, ho, hl = HH.ms_build(batch, DEV, sclm)
    if not matching:
        ho.pop("lowest_cost")
    for f, s_ in ((-1, "m1"), (1, "p1")):
        hm[("axisangle", 0, f)] = hl["axisangle_" + s_]
        hm[("translation", 0, f)] = hl["translation_" + s_]
    losses, mono_losses, decs = step.loss_step_multiscale(trainer.default_options(**kw), hi, hm, ho, noises=[n.to(DEV) for n in nt],
                                                          want_decisions=True)
    losses["loss"].backward()
    torch.cuda.synchronize()
    lo = {k: float(v.detach()) for k, v in losses.items()}
    lo.update({"mono/" + k: float(v.detach()) for k, v in mono_losses.items()})
    planes = {"%s%d" % (k, s): torch.as_tensor(v[s]).cpu() for k, v in decs.items() for s in range(sclm + 1)}
    return lo, planes, {k: t.grad.cpu().numpy() for k, t in hl.items()}


def test_four_scale_decomposition_sweep():
    from mal_amd.synthetic import make_batch
    from tests.test_gpu_multiscale import check_multiscale_decision_exact
    B, H, W, sclm = 2, 40, 136, 3
    batch = make_batch(B, H, W, seed=79)
    g = torch.Generator().manual_seed(12)
    nt = [torch.randn(B, 1, H, W, generator=g) for _ in range(sclm + 1)]
    kw = dict(height=H, width=W, batch_size=B, sclm=sclm, distil=False)
    ref = _ms_run(batch, kw, nt)
    for cfg in decomposition_configs(H):
        set_options(march_rows=0, march_rows_fwd=0, pack_rows=10, syn_rows=4, march_halo1=1, march_flip=1, device_cus=0)
        set_options(**cfg)
        _hold_like_default(_ms_run(batch, kw, nt), ref, cfg)
    set_options(march_rows=9, march_rows_fwd=11, pack_rows=17, syn_rows=3, march_halo1=1, march_flip=0, device_cus=0)
    counts, report = check_multiscale_decision_exact(batch, kw, nt, True)
    assert all(v[0] <= 1e-4 for v in report.values()), report


# ---- DualRefine's one-call step: upstream's scales [0, 1, 2, 3]; the pose-update losses

def _dr_scales_run():
    from mal_amd import dualrefine, layers
    z = G.load("dualrefine_b2_40x72_scales0123")
    b, scales, units, inputs, outputs, leaves = G.dualrefine_dicts(z, layers.transformation_from_parameters, DEV)
    B, _, H, W = b["color0"].shape
    torch.manual_seed(int(z["in/noise_seed"]))
    noises = [torch.randn(B, 1, H, W).to(DEV) for _ in units]
    lp = dualrefine.DualRefineLossPath(dualrefine.default_options(height=H, width=W, batch_size=B, n_losses=1, scales=scales), fuse=True)
    got, decs = lp.loss_step(inputs, outputs, noises=noises, want_decisions=True)
    got["loss"].backward()
    torch.cuda.synchronize()
    return ({k: float(v.detach()) for k, v in got.items()}, {str(k): torch.as_tensor(v).cpu() for k, v in decs.items()},
            {k: t.grad.cpu().numpy() for k, t in leaves.items()})


def test_dualrefine_decomposition_sweep():
    from tests.test_gpu_decisions import test_dualrefine_pose_update_losses_in_the_one_call_step as pose_update_case
    ref = _dr_scales_run()
    for cfg in decomposition_configs(40):
        set_options(march_rows=0, march_rows_fwd=0, pack_rows=10, syn_rows=4, march_halo1=1, march_flip=1, device_cus=0)
        set_options(**cfg)
        _hold_like_default(_dr_scales_run(), ref, cfg)
    # the pose-update pass through the decision-exact check against the forced oracle, gates unchanged
    for cfg in ({"march_rows": 9, "march_flip": 0, "pack_rows": 17}, {"device_cus": 1, "march_halo1": 0}):
        set_options(march_rows=0, march_rows_fwd=0, pack_rows=10, syn_rows=4, march_halo1=1, march_flip=1, device_cus=0)
        set_options(**cfg)
        pose_update_case((3, 37, 50), {"Tstar_D0_pair": True})


# ---- the baseline size as benchmarked, decompositions of other devices

def test_baseline_size_on_other_device_sizes():
    """B=12 192x640 --temporal --distil with the real producer: "device_cus" 32 (one CPX partition: every strip is ONE
    segment, no halo or boundary scratch row is used) and 304 (MI300X: 11 rows).  Both give the default's decision planes bit
    for bit; the 32-CU run is decision-exact against the oracle (one oracle run for the three), and the 304-CU step replayed
    from a captured graph equals the same step run eagerly bit for bit."""
    from mal_amd import _lib as L
    from mal_amd.synthetic import make_batch
    from tests.test_gpu_decisions import check_step_decision_exact
    B, H, W = 12, 192, 640
    lib = _lib()
    geo = {}
    for cus in (32, 304):
        set_options(device_cus=cus)
        s, g_, r = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        L.check(lib.mal_march_geometry(B, H, W, 2, ctypes.byref(s), ctypes.byref(g_), ctypes.byref(r), None), "geometry")
        geo[cus] = (g_.value, r.value)
    assert geo[32] == (1, 192) and geo[304] == (18, 11), geo
    b = make_batch(B, H, W, seed=1234)
    b["syn_instances"] = (3, 1234)
    g = torch.Generator().manual_seed(8)
    n0, n1 = torch.randn(B, 1, H, W, generator=g), torch.randn(B, 1, H, W, generator=g)
    set_options(device_cus=0)
    ref = _step_run(b, {"temporal": True}, n0)
    set_options(device_cus=304)
    _hold_like_default(_step_run(b, {"temporal": True}, n0), ref, {"device_cus": 304})
    set_options(device_cus=32)
    (h, o), counts, report = check_step_decision_exact(b, {"temporal": True}, n0, n1, return_runs=True)
    _hold_like_default((h["losses"], {k: h["maps"][k] for k in ("dec_teacher", "dec_student")}, h["grads"]), ref, {"device_cus": 32})
    set_options(device_cus=304)
    eager, graph = _bench_runs("step", False, True)
    for (l0, g0), (l1, g1) in zip(eager, graph):
        assert l0 == l1
        assert set(g0) == set(g1) and all(torch.equal(g0[k], g1[k]) for k in g0)


# ---- pure scheduling switches: bitwise, eager and graph-replayed

def _bench_runs(mode, main_temporal, graph_too, steps=3):
    """bench.Step at the baseline size: losses and gradients of `steps` steps, eager and (graph_too) replayed from a graph"""
    import bench
    from mal_amd import config
    from mal_amd import step as step_mod
    dev = torch.device(DEV)
    old_noise = config.noise_source, config.noise_seed
    out = []
    try:
        for graph in ((False, True) if graph_too else (False,)):
            step = bench.Step(dev, 4321, mode, main_temporal=main_temporal)
            step_mod.noise_counter(dev).zero_()  # the in-kernel tie-break noise: the same draws for every run
            runs = []
            with torch.cuda.stream(torch.cuda.Stream()):
                for _ in range(2):
                    step()
                torch.cuda.synchronize()
                step_mod.noise_counter(dev).zero_()
                if graph:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=torch.cuda.current_stream()):
                        loss = step()
                    step_mod.noise_counter(dev).zero_()
                for _ in range(steps):
                    if graph:
                        g.replay()
                    else:
                        loss = step()
                    torch.cuda.synchronize()
                    runs.append((float(loss.detach()), {k: t.grad.detach().clone() for k, t in step.leaves.items() if t.grad is not None}))
            out.append(runs)
    finally:
        config.noise_source, config.noise_seed = old_noise
    return out


# (name, value, mode, --main_temporal, the reference's options).  "step_overlap" != 1 also turns the tail overlap off (it
# needs the side stream's fork of value 1): the teacher's sweep then finishes d total / d disp_teacher itself instead of the
# assembly, one fused multiply-add associated differently (tests/test_gpu_step.py::test_tail_overlap_equals_the_serial_backward
# holds that difference), so its reference is the default schedule with "tail_overlap" 0 -- against which it is bitwise
SWITCHES = [("step_overlap", 0, "step", False, {"tail_overlap": 0}), ("step_overlap", 2, "step", False, {"tail_overlap": 0}),
            ("student_overlap", 0, "step", False, {}), ("side_order", 1, "step", False, {}),
            ("sweeps_batched", 0, "step", True, {}), ("ms_fold", 0, "multiscale", False, {})]
_DEFAULT_RUNS = {}


@pytest.mark.parametrize("name,value,mode,main_temporal,ref_opts", SWITCHES, ids=["%s=%d" % (s[0], s[1]) for s in SWITCHES])
def test_scheduling_switch_is_bitwise(name, value, mode, main_temporal, ref_opts):
    key = (mode, main_temporal, tuple(sorted(ref_opts.items())))
    if key not in _DEFAULT_RUNS:
        set_options(**ref_opts)
        _DEFAULT_RUNS[key] = _bench_runs(mode, main_temporal, True)
    ref = _DEFAULT_RUNS[key]
    set_options(**ref_opts)
    set_options(**{name: value})
    got = _bench_runs(mode, main_temporal, True)
    for how, r_runs, g_runs in zip(("eager", "graph"), ref, got):
        for (l0, g0), (l1, g1) in zip(r_runs, g_runs):
            assert l0 == l1, (name, value, how, l0, l1)
            assert set(g0) == set(g1)
            for k in g0:
                assert torch.equal(g0[k], g1[k]), (name, value, how, k)


def _child_main(name, value):
    """(in a fresh process) set the option before any step, then print the eager and graph-replayed runs' losses and gradients"""
    set_options(**{name: value})
    for how, runs in zip(("eager", "graph"), _bench_runs("step", False, True)):
        for loss, grads in runs:
            print("RUN", how, loss.hex(), " ".join("%s:%s" % (k, hash(grads[k].cpu().numpy().tobytes())) for k in sorted(grads)))


def test_side_priority_is_bitwise_in_a_fresh_process():
    """"side_priority" is read when a caller stream's side stream is first created: each value in a process of its own"""
    res = {}
    for v in (0, 1):
        code = "from tests.test_gpu_schedule import _child_main; _child_main('side_priority', %d)" % v
        p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, PYTHONHASHSEED="0"))
        assert p.returncode == 0, (v, p.stdout[-2000:], p.stderr[-2000:])
        res[v] = [l for l in p.stdout.splitlines() if l.startswith("RUN ")]
        assert len(res[v]) == 6, p.stdout[-2000:]
    assert res[0] == res[1]


# ---- the N4 VJPs under every plane formulation

@pytest.mark.parametrize("planes", [0, 1])
def test_epipolar_vjps_under_epi_bwd_planes(planes):
    from tests import test_gpu_epipolar as E
    set_options(epi_bwd_planes=planes)
    for tag in ("epi_grad_b2_c16_12x20_r4_l3", "epi_grad_b1_c8_9x13_r2_l2_h2"):
        E.test_lookup_vjp_golden(tag)
    for t in ("epi_aligngrad_b2_c16_12x20_r4_l3", "epi_aligngrad_b1_c8_9x13_r2_l2_h2"):
        for r in ("", "_robust"):
            E.test_direct_align_vjp_golden(t + r)
    E.test_lookup_vjp_dualrefine_size()
    for robust in (False, True):
        E.test_direct_align_vjp_pieces_dualrefine_size(robust)


# ---- options changed between a step's forward and its backward

def _change_between(fwd, option, value):
    """run fwd() -> loss, set the option, backward: refused with MalError (the step's boundary rows and partials need the
    decomposition its forward used)"""
    from mal_amd import _lib as L
    loss = fwd()
    set_options(**{option: value})
    with pytest.raises(L.MalError, match="decomposition"):
        loss.backward()
    torch.cuda.synchronize()


@pytest.mark.parametrize("option,value", [("march_rows", 9), ("device_cus", 1)])
def test_step_backward_refuses_a_changed_decomposition(option, value):
    from mal_amd import step, trainer
    from mal_amd.synthetic import make_batch, to_dicts
    B, H, W = 2, 40, 130

    def fwd():
        set_options(march_rows=0, device_cus=0)
        b = make_batch(B, H, W, seed=3)
        inputs, mono_outputs, outputs, leaves = to_dicts(b, lambda a, t, inv: None, device=torch.device(DEV))
        for f, s in ((-1, "m1"), (1, "p1")):
            mono_outputs[("axisangle", 0, f)] = leaves["axisangle_" + s]
            mono_outputs[("translation", 0, f)] = leaves["translation_" + s]
        losses, _, _ = step.loss_step(trainer.default_options(height=H, width=W, batch_size=B), inputs, mono_outputs, outputs,
                                      want_maps=False)
        return losses["loss"]
    _change_between(fwd, option, value)
    # the library is still usable: an unchanged step goes through
    loss = fwd()
    loss.backward()
    torch.cuda.synchronize()


@pytest.mark.parametrize("option,value", [("march_rows", 9), ("device_cus", 1)])
def test_four_scale_backward_refuses_a_changed_decomposition(option, value):
    from mal_amd import step, trainer
    from mal_amd.synthetic import make_batch
    B, H, W, sclm = 2, 40, 136, 3

    def fwd():
        set_options(march_rows=0, device_cus=0)
        batch = make_batch(B, H, W, seed=79)
        hi, hm, ho, hl = HH.ms_build(batch, DEV, sclm)
        for f, s_ in ((-1, "m1"), (1, "p1")):
            hm[("axisangle", 0, f)] = hl["axisangle_" + s_]
            hm[("translation", 0, f)] = hl["translation_" + s_]
        nt = [torch.randn(B, 1, H, W, device=DEV) for _ in range(sclm + 1)]
        losses, _ = step.loss_step_multiscale(trainer.default_options(height=H, width=W, batch_size=B, sclm=sclm, distil=False),
                                              hi, hm, ho, noises=nt)
        return losses["loss"]
    _change_between(fwd, option, value)
    loss = fwd()
    loss.backward()
    torch.cuda.synchronize()


@pytest.mark.parametrize("option,value", [("march_rows", 9), ("device_cus", 1)])
def test_dualrefine_backward_refuses_a_changed_decomposition(option, value):
    from mal_amd import dualrefine, layers
    from mal_amd.synthetic import make_batch
    from tests.test_gpu_decisions import _dr_build_pu
    B, H, W = 3, 37, 50

    def fwd():
        set_options(march_rows=0, device_cus=0)
        batch = make_batch(B, H, W, seed=324)
        inputs, outputs, gl = _dr_build_pu(batch, DEV, layers.transformation_from_parameters)
        lp = dualrefine.DualRefineLossPath(dualrefine.default_options(disable_pose_updates=False, height=H, width=W, batch_size=B,
                                                                      n_losses=1), fuse=True)
        got = lp.loss_step(inputs, outputs, noises=[torch.randn(B, 1, H, W, device=DEV) for _ in range(2)],
                           pose_noise=torch.randn(B, 1, H, W, device=DEV))
        return got["loss"]
    _change_between(fwd, option, value)
    loss = fwd()
    loss.backward()
    torch.cuda.synchronize()
