"""CPU: --distil with --scales 0 1 2 3 in the one-call step -- the C entry point of the extra scales' warps rejects bad
arguments before any device work, and the CPU oracle reproduces the reference-generated fixtures
(scripts/gen_golden_step_scales.py) bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from mal_amd.synthetic import to_dicts, fake_image_synthesis
from oracle import mal_oracle as O
from tests import golden_io as G

SCALE_CASES = ["step_b2_48x96_sclm3_temporal", "step_b2_48x96_sclm3_temporal_main", "step_b2_48x96_sclm3_lastnone"]


def producer_of(z, b):
    """the fixture's producer: the stand-in of the other fixtures, or (``lastnone``) the same except that its call at the
    last scale writes nothing and reports no instance"""
    synth = fake_image_synthesis(b["syn_rects"])
    if str(z["producer"]) == "lastnone":
        last = int(z["sclm"])
        return lambda inputs, outputs, scale: False if scale == last else synth(inputs, outputs, scale)
    return synth


def scale_dicts(z, pose_fn, device=None):
    """a fixture as the reference's dicts: ("disp", s) of both networks for s = 0..sclm (the lower scales are leaves of
    their own, ``disp_teacher_s1`` ...)"""
    b = G.batch_from_golden(z)
    inputs, mono_outputs, outputs, leaves = to_dicts(b, pose_fn, device=device)
    for s in range(1, int(z["sclm"]) + 1):
        for name, outs in (("disp_teacher", mono_outputs), ("disp_student", outputs)):
            leaf = torch.from_numpy(z["in/%s_s%d" % (name, s)].astype(np.float32)).to(device or "cpu").requires_grad_(True)
            leaves["%s_s%d" % (name, s)] = leaf
            outs[("disp", s)] = leaf
    return b, inputs, mono_outputs, outputs, leaves


def summary_matches(name, t, z, tol=0.0):
    """``t`` against what oracle.gen_golden.summarize recorded (sums of the whole tensor, the 8x8-strided subsample)"""
    a = t.detach().double().cpu()
    for k, v in (("#sum", a.sum()), ("#abs", a.abs().sum()), ("#sq", (a * a).sum())):
        ref = float(z[name + k])
        assert abs(float(v) - ref) <= tol * max(1.0, abs(ref)), (name + k, float(v), ref)
    sub = t.detach()[..., ::8, ::8].cpu().numpy()
    assert np.abs(sub - z[name + "#sub"]).max() <= tol, name + "#sub"


def run_oracle(z):
    b, inputs, mono_outputs, outputs, leaves = scale_dicts(z, O.transformation_from_parameters)
    B, _, H, W = b["color0"].shape
    opt = O.default_opt(height=H, width=W, batch_size=B, **G.opt_kwargs(z))
    n0 = torch.from_numpy(z["in/noise_mono"].copy())
    n1 = torch.from_numpy(z["in/noise_main"].copy())
    losses, _, mono_losses, _, _ = O.mal_loss_step(opt, inputs, mono_outputs, outputs, n0, n1, [0.7, 0.3],
                                                   synth=producer_of(z, b))
    losses["loss"].backward()
    return losses, mono_losses, mono_outputs, outputs, leaves


@pytest.mark.parametrize("tag", SCALE_CASES)
def test_oracle_reproduces_the_reference_with_four_scales(tag):
    """sclm = 3 with --distil: generate_images_pred warps every scale and calls the producer on each (trainer.py:1088-1165),
    the losses read scale 0 only, has_ins is the last call's -- the oracle's loop reproduces the fixture bit for bit"""
    z = G.load(tag)
    losses, mono_losses, mono_outputs, outputs, leaves = run_oracle(z)
    assert float(losses["loss"].detach()) == float(z["final_loss"])
    for k, v in losses.items():
        assert float(v.detach()) == float(z["losses/" + k]), k
    for k, v in mono_losses.items():
        assert float(v.detach()) == float(z["mono_losses/" + k]), k
    for k, t in leaves.items():
        g = t.grad if t.grad is not None else torch.zeros_like(t)
        assert np.array_equal(g.numpy(), z["grad/" + k]), k
        if k[-3:] in ("_s1", "_s2", "_s3"):  # no loss reads the lower scales
            assert not z["grad/" + k].any(), k
    for who, outs in (("mono", mono_outputs), ("multi", outputs)):
        for s in range(1, int(z["sclm"]) + 1):
            for f, fn in ((-1, "m1"), (1, "p1")):
                for kind in ("color", "syn"):
                    name = "%s/%s_%s_s%d" % (who, kind, fn, s)
                    if name + "#sum" in z:
                        summary_matches(name, outs[(kind, f, s)], z)
                    else:
                        assert (kind, f, s) not in outs or who == "multi", name


def test_lastnone_fixture_drops_the_synthesised_candidates():
    """the producer's call at scale 3 reports no instance: upstream then takes the min over the two warped candidates only,
    whatever scale 0 returned -- the fixture must show it"""
    z = G.load("step_b2_48x96_sclm3_lastnone")
    assert int(z["has_ins"]) == 0
    zt = G.load("step_b2_48x96_sclm3_temporal")
    assert int(zt["has_ins"]) == 1


# ------------------------------------------------------------------ the C entry point's argument checks (no device)
@pytest.fixture(scope="module")
def lib():
    from mal_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_warp_scales_is_exported_with_its_struct(lib):
    from mal_amd import _lib
    assert "mal_loss_step_warp_scales" in _lib.SIGNATURES
    assert lib.mal_struct_bytes(4) == C.sizeof(_lib.StepScalesArgs)


def test_warp_scales_rejects_bad_arguments_without_a_device(lib):
    from mal_amd import _lib as L
    fake = 0x1000  # never dereferenced: every check below fails before any device work

    def args(B=2, H=48, W=96, flags=L.STEP_TEMPORAL):
        a = L.StepArgs()
        a.B, a.H, a.W, a.flags = B, H, W, flags
        return a

    def scales(sclm=3, student=False, warp2=None):
        s = L.StepScalesArgs()
        s.sclm = sclm
        for k in range(1, 4):
            s.disp_teacher[k] = s.disp_student[k] = fake
            s.warp_m1[k] = s.warp_p1[k] = s.warp_s_m1[k] = s.warp_s_p1[k] = fake
        if warp2 is not None:
            s.warp2_m1[warp2] = fake  # one of a pair
        return s

    call = lambda a, s: lib.mal_loss_step_warp_scales(C.byref(a) if a is not None else None, C.byref(s) if s is not None else None)
    EINVAL, ESHAPE = -1, -2
    assert call(None, scales()) == EINVAL
    assert call(args(), None) == EINVAL
    for sclm in (0, 4, -1):
        assert call(args(), scales(sclm)) == EINVAL, sclm
    assert call(args(H=50), scales(3)) == ESHAPE   # 50 % 8
    assert call(args(W=100), scales(3)) == ESHAPE  # 100 % 8
    assert call(args(H=50), scales(1)) == EINVAL   # divisible by 2: on to the (null) step arguments
    assert call(args(flags=0), scales()) == EINVAL  # no hinted pass
    s = scales()
    s.disp_teacher[2] = None
    assert call(args(), s) == EINVAL
    s = scales()
    s.warp_s_p1[3] = None
    assert call(args(flags=L.STEP_MAIN_TEMPORAL), s) == EINVAL
    assert call(args(flags=L.STEP_TEMPORAL), s) == EINVAL  # (the student's warps are not read: null step arguments)
    assert call(args(), scales(warp2=2)) == EINVAL
    s = scales(1)
    s.disp_teacher[2] = None  # scales above sclm are not read
    assert call(args(), s) == EINVAL  # ... it fails on the step arguments (null colours, workspace)
