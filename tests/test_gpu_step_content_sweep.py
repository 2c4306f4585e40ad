"""The one-call loss steps (mal_loss_step_*, mal_loss_multiscale_*, mal_dr_loss_*) on hostile batch CONTENT
(tests/step_content_cases.py): per-sample intrinsics, large motion, points behind the camera, both ends of the depth range,
flat images, samples and batches without a live student weight.  tests/test_step_content_cases.py shows on the CPU that every
case reaches its edge and that the reference alone meets the gates there; here the marching kernels are held to the same
gates, through the checkers of the other step tests, unchanged: no tolerance is new."""
import numpy as np
import pytest
import torch

from tests import hip_harness as HH
from tests import step_content_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


def _id(shape):
    return "b%d_%dx%d" % tuple(shape)


def _hold_plain(name, shape, report):
    """1e-4 plain (L2 rel to the fp64 forced oracle) on every leaf, as the other small-shape tests ask; where the fp32 oracle
    ITSELF is above 8e-5 (C.FLOOR_LEAVES: translation_m1 of flat_images at (2, 24, 72), 9.0e-5) the checker's own
    max(1e-4, 1.25 x floor) stands, which it has asserted already"""
    own_floor = C.FLOOR_LEAVES.get((name, tuple(shape)), ())
    assert all(v[0] <= 1e-4 for k, v in report.items() if k not in own_floor), report


def _single(name, shape, kw, with_syn=False, scalars=True):
    from tests.test_gpu_decisions import check_step_decision_exact
    from tests.test_gpu_step import _check_step
    b, n0, n1 = C.case(name, shape, with_syn=with_syn)
    counts, report = _check_step(b, kw, n0, n1) if scalars else check_step_decision_exact(b, kw, n0, n1)
    print("content sweep %s %s %s: differing decisions %s; L2 rel to fp64 (hip, fp32 oracle) %s"
          % (name, _id(shape), kw, {k: v for k, v in counts.items() if v}, {k: "%.1e/%.1e" % v for k, v in report.items()}))
    _hold_plain(name, shape, report)


@pytest.mark.parametrize("shape", C.SHAPES, ids=_id)
@pytest.mark.parametrize("name", C.VARIANTS)
def test_single_scale_step(name, shape):
    """decision-exact gradients (check_step_decision_exact) and the free-running scalars and maps (_check_step, which runs it)"""
    _single(name, shape, {})


@pytest.mark.parametrize("shape", C.SHAPES, ids=_id)
@pytest.mark.parametrize("kw", [{"temporal": True}, {"temporal": True, "main_temporal": True}], ids=["temporal", "both"])
@pytest.mark.parametrize("name", C.GEOMETRY)
def test_single_scale_step_with_the_temporal_hint(name, kw, shape):
    """the exporting passes, the materialised-candidate sweeps, the sparse cotangent and the FRAMED instantiations on the
    geometry cases (as the other temporal tests: decision-exact; the free-running scalars are the plain step's matter)"""
    _single(name, shape, kw, with_syn=True, scalars=False)


@pytest.mark.parametrize("shape", C.SHAPES, ids=_id)
@pytest.mark.parametrize("name", C.DEAD)
def test_single_scale_step_without_the_ensemble_pass(name, shape):
    _single(name, shape, {"no_ens": True})


@pytest.mark.parametrize("shape", C.SHAPES, ids=_id)
def test_per_sample_K_discriminates(shape):
    """the step on the batch with K[0] handed to every sample -- what a camera block filled from `K + 0` would compute -- is
    further from the per-sample step than 100 x the gate of the loss scalars (1e-5 relative): the CPU table's condition, on the
    device's own numbers"""
    from tests.test_gpu_step import run_step
    b, n0, n1 = C.case("per_sample_K", shape)
    a, c = run_step(b, {}, n0), run_step(C.broadcast_K0(b), {}, n0)
    assert abs(c["losses"]["loss"] - a["losses"]["loss"]) > 100 * 1e-5 * abs(a["losses"]["loss"]), (a["losses"]["loss"], c["losses"]["loss"])


@pytest.mark.parametrize("shape", C.SHAPES, ids=_id)
def test_dead_weights_all(shape):
    """Every student weight dead (consistency x matching; augmentation 0): 0 / (0 + 1e-7) and its gradient.

    What is exactly zero is the student's PHOTOMETRIC share.  Its disparity still collects the consistency term, whose weight
    1 - 0 is then 1 everywhere, and its smoothness term (oracle: compute_main_losses; tests/test_step_content_cases.py shows that
    the oracle's disp_student gradient is the gradient of those two alone and is not zero), so `disp_student.grad == 0` does not
    hold for the reference.  Held instead: the student's reprojection and distillation scalars are exactly 0; disp_student's
    gradient does not change by one bit when the two source frames change places -- nothing photometric reaches it; the pose
    gradients, which the student's and the ensemble's passes never reach (their poses are detached), equal the teacher-only
    ones of the --no_ens oracle within the gradient gate; nothing is NaN.  (The gates of test_single_scale_step hold the rest.)"""
    from tests.test_gpu_decisions import _l2rel, _to64, run_step_with_decisions
    b, n0, n1 = C.case("dead_weights_all", shape)
    h = run_step_with_decisions(b, {}, n0)
    assert all(np.isfinite(v) for v in h["losses"].values()) and all(np.isfinite(g).all() for g in h["grads"].values())
    assert h["losses"]["distil_loss"] == 0.0
    assert h["losses"]["reproj_loss/0"] == h["losses"]["mono/reproj_loss/0"]  # teacher's + 0
    assert np.abs(h["grads"]["disp_student"]).max() > 0
    swapped = dict(b, color_m1=b["color_p1"], color_p1=b["color_m1"])
    s = run_step_with_decisions(swapped, {}, n0)
    assert not np.array_equal(s["grads"]["disp_teacher"], h["grads"]["disp_teacher"])  # the swap does change the photometric terms
    assert np.array_equal(s["grads"]["disp_student"], h["grads"]["disp_student"])
    kd = HH.kernel_decisions(h["maps"])
    f32 = HH.run_oracle(b, {"no_ens": True}, n0, n1, forced=kd)
    f64 = HH.run_oracle(C.to64(b), {"no_ens": True}, n0.double(), n1.double(), forced=_to64(kd))
    for k in HH.LEAVES[2:]:
        r32, r64 = f32["grads"][k], f64["grads"][k]
        assert _l2rel(h["grads"][k], r64) <= max(1e-4, 1.25 * _l2rel(r32, r64)), (k, _l2rel(h["grads"][k], r64), _l2rel(r32, r64))


@pytest.mark.parametrize("shape", C.SHAPES, ids=_id)
@pytest.mark.parametrize("name", C.GEOMETRY)
def test_both_routes_agree(name, shape):
    """the marching warp of the one-call step and the pixel warp of the operator route on clipped and behind-camera samples:
    2e-6 on the loss, 2e-5 of its scale on every gradient"""
    from tests.test_gpu_step import check_step_equals_operator_route
    b, n0, n1 = C.case(name, shape)
    check_step_equals_operator_route(b, {}, n0, n1)


@pytest.mark.parametrize("name,temporal", [(n, False) for n in C.MS_GEOMETRY] + [("large_motion", True)],
                         ids=list(C.MS_GEOMETRY) + ["large_motion-temporal"])
def test_four_scale_step(name, temporal):
    """mal_loss_multiscale_* at (3, 40, 72), sclm 2, with the matching mask; without the temporal hint, and large_motion with it"""
    from mal_amd.synthetic import fake_image_synthesis
    from tests.test_gpu_multiscale import check_multiscale_decision_exact
    B, H, W = C.MS_SHAPE
    sclm = C.MS_SCLM
    b, n0, n1 = C.case(name, C.MS_SHAPE, with_syn=temporal)
    g = torch.Generator().manual_seed(12)
    nt = [torch.randn(B, 1, H, W, generator=g) for _ in range(sclm + 1)]
    kw = dict(height=H, width=W, batch_size=B, sclm=sclm, distil=False, temporal=temporal)
    counts, report = check_multiscale_decision_exact(b, kw, nt, True, (lambda: fake_image_synthesis(b["syn_rects"])) if temporal else None)
    print("content sweep four scales %s: differing decisions %s" % (name, {k: v for k, v in counts.items() if v}))
    assert all(v[0] <= 1e-4 for v in report.values()), report


@pytest.mark.parametrize("name", C.GEOMETRY)
def test_dualrefine_step_decision_exact(name):
    """convention 1 (align_corners=False), a branch of its own in the projection tail"""
    from tests.test_gpu_decisions import check_dualrefine_decision_exact
    check_dualrefine_decision_exact(C.case(name, C.DR_SHAPE)[0])


@pytest.mark.parametrize("name", C.GEOMETRY)
def test_dualrefine_one_call_step_equals_the_operator_route(name):
    from tests.test_gpu_decisions import check_dualrefine_step_equals_the_operator_route
    check_dualrefine_step_equals_the_operator_route(C.case(name, C.DR_SHAPE)[0], {})


@pytest.mark.parametrize("name", C.GEOMETRY)
def test_dualrefine_pose_update_step_against_the_oracle_and_the_operator_route(name):
    """the pose-update pass (FRAMED: two candidates with two disparities and two poses) on the geometry cases: decision-exact
    against the oracle, and against the operator route of the same term"""
    from tests.test_gpu_decisions import check_dualrefine_pose_update_step
    from tests.test_gpu_decisions import check_dualrefine_step_equals_the_operator_route
    check_dualrefine_pose_update_step(C.case(name, C.DR_SHAPE)[0], {})
    check_dualrefine_step_equals_the_operator_route(C.case(name, C.DR_SHAPE)[0], {}, pose_update=True)
