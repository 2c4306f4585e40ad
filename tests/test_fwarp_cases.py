"""CPU: the checker of mal_amd.rigid_warp (tests/fwarp_restated.py) against the reference's own outputs
(tests/golden/fwarp_*.npz, scripts/gen_golden_fwarp.py), the gates of the GPU tests applied to the reference's own
arithmetic, the launch plan and the host refusals.  Nothing is launched.

Gates (tests/fwarp_restated.py has the checkers).  Decisions -- the cell a sub-point truncates to, and iw_val -- are taken
from the restatement in fp64.  fp32 may take another decision at no more than 3e-4 N + 8 places (N sub-points; the
project's cap), and only where the fp64 value is a near-tie: x or y within 1e-4 of a truncation edge (-1, 1, 2, ..., W; 0 is
no edge), |coord| within 1e-5 of 1.  A fixture that cannot hold these with the reference's own arithmetic would be a
wrong fixture: its seed is replaced, nothing is widened."""
import ctypes

import numpy as np
import pytest
import torch

from tests import fwarp_restated as R

DECISION_CASES = [k for k in R.CASES if R.CASES[k][5] != "identity"]


@pytest.fixture(scope="module")
def lib():
    from mal_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("name", R.GOLDEN_CASES)
def test_restatement_is_the_reference_bit_for_bit(name):
    g, c = R.load_golden(name), R.make_case(name)
    for k in ("img", "depth", "pose", "K"):
        assert np.array_equal(bits(g[k]), bits(c[k].numpy())), "the case table no longer produces the fixture's %s" % k
    assert int(g["up"]) == c["up"]
    r = R.forward_warp(c["img"], c["depth"], c["pose"], c["K"], c["up"], torch.float32)
    for k in ("img_w", "depth_w", "valid"):
        assert r[k].dtype == torch.float32 and np.array_equal(bits(g[k]), bits(r[k].numpy())), k


@pytest.mark.parametrize("name", DECISION_CASES)
def test_reference_arithmetic_meets_the_gates(name):
    c = R.make_case(name)
    B, _, H, W = c["depth"].shape
    s32 = R.splat(c["depth"], c["pose"], c["K"], c["up"], torch.float32)
    s64 = R.splat(c["depth"], c["pose"], c["K"], c["up"], torch.float64)
    N = s64["cell"].numel()
    n_cells = R.check_cells(s32, s64, H, W)
    n_z, gate = R.check_zbuf(s32["zbuf"].numpy(), s32, s64, H, W)
    # stage 2 on ONE z-buffer, the fp32 one, so that its decisions are judged alone
    r32 = R.resolve(s32["zbuf"], c["img"], c["pose"], c["K"], torch.float32)
    r64 = R.resolve(s32["zbuf"], c["img"], c["pose"], c["K"], torch.float64)
    rep = R.check_resolve({k: r32[k].numpy() for k in ("img_w", "depth_w", "valid")}, r32, r64, 1.0, N)
    holes = float((s64["zbuf"] == 0).double().mean())
    print("%s: N %d, differing cells %d, differing z cells %d (gate %.2g), valid %d, depth_w %.2g rel, img_w %.2g, holes %.0f %%"
          % (name, N, n_cells, n_z, gate, rep["valid_diff"], rep["depth_rel"], rep["img"], 100 * holes))
    kind = R.CASES[name][5]
    if kind == "all_outside":
        assert holes == 1.0 and not r64["img_w"].any() and not r64["depth_w"].any() and not r64["valid"].any()
    if kind == "generic" and H * W >= 35:
        assert 0.05 < holes < 0.6
    if kind == "diverge":
        assert holes > 0.5
    if kind == "converge":
        assert float((s64["cell"] >= 0).sum()) / max(1.0, float((s64["zbuf"] != 0).sum())) > 12  # sub-points per filled cell
    if kind == "behind_camera":
        assert (s64["inv"] == 1000.0).double().mean() > 0.2 and (s64["zbuf"] == 1000.0).double().mean() > 0.05
    if kind == "parallax_split":
        shift = (s64["x"].reshape(B, H * c["up"], W * c["up"]) - (torch.arange(W * c["up"], dtype=torch.float64) + 0.0) / c["up"]).abs()
        assert (shift > W / 4).double().mean() > 0.3 and (shift < 1).double().mean() > 0.3
    if kind == "large_motion":
        x, y = s64["x"], s64["y"]
        assert (x <= -1).any() and (x >= W).any() and (y <= -1).any() and (y >= H).any()


def test_identity_pose_is_not_a_decision_case():
    """With a generic K and the identity pose every sub-point whose coordinate is a multiple of up projects onto the pixel
    lattice, i.e. ON a truncation edge: fp32 and fp64 then round to different sides with no kernel involved.  With a
    power-of-two K (and depths that are powers of two) the cells agree, yet the warped image is still not bit-equal, so no
    case is held EQUAL to fp64."""
    c = R.make_case("lattice_generic_u3")
    B, _, H, W = c["depth"].shape
    s32 = R.splat(c["depth"], c["pose"], c["K"], 3, torch.float32)
    s64 = R.splat(c["depth"], c["pose"], c["K"], 3, torch.float64)
    N = s64["cell"].numel()
    differ = int((s32["cell"] != s64["cell"]).sum())
    print("lattice_generic_u3: %d of %d sub-point cells differ between fp32 and fp64" % (differ, N))
    assert N == 31104 and differ > 10 * R.cap(N)
    with pytest.raises(AssertionError, match="cells differ"):
        R.check_cells(s32, s64, H, W)
    # ... and every one of them is a lattice point, which the near-tie rule would wave through: the gate would decide nothing
    tie = R.near_edge(s64["x"].numpy(), W) | R.near_edge(s64["y"].numpy(), H)
    assert tie.mean() > 0.3
    for up in (1, 2, 3, 4):
        c = R.make_case("lattice_pow2_u%d" % up)
        r32 = R.forward_warp(c["img"], c["depth"], c["pose"], c["K"], up, torch.float32)
        r64 = R.forward_warp(c["img"], c["depth"], c["pose"], c["K"], up, torch.float64)
        assert torch.equal(r32["splat"]["cell"], r64["splat"]["cell"]), up
        assert not torch.equal(r32["img_w"].double(), r64["img_w"]), up


def test_nearest_upsampling_is_integer_division():
    """F.interpolate(scale_factor=up) is what forward_warp upsamples the depth with (:561); the kernel reads
    depth[v // up][u // up].  Equal for up = 2..5 and every length 1..2048 (ATen computes the source index in float)."""
    for up in (2, 3, 4, 5):
        for n in range(1, 2049):
            src = torch.arange(n, dtype=torch.float32).view(1, 1, 1, n)
            got = torch.nn.functional.interpolate(src, scale_factor=(1, up))[0, 0, 0]
            assert torch.equal(got, torch.div(torch.arange(n * up), up, rounding_mode="floor").float()), (up, n)
    src = torch.arange(6, dtype=torch.float32).view(1, 1, 2, 3)
    got = torch.nn.functional.interpolate(src, scale_factor=3)[0, 0]
    assert torch.equal(got, src[0, 0][torch.arange(6)[:, None] // 3, torch.arange(9)[None] // 3])


def plan(lib, B, C, H, W, up, P):
    from mal_amd import ops
    return ops.forward_warp_plan(B, C, H, W, up, P)


@pytest.mark.parametrize("name", list(R.CASES))
def test_plan_covers_every_case(lib, name):
    B, H, W, C, up = R.CASES[name][:5]
    for P in (1, 2):
        p = plan(lib, B, C, H, W, up, P)
        assert (p["vec"], p["tile_w"], p["tile_h"], p["lds_bytes"]) == (1, 64, 4, 0)
        assert p["tiles_x"] == -(-W // 64) and p["tiles_y"] == -(-H // 4)
        assert p["tiles_x"] * 64 >= W > (p["tiles_x"] - 1) * 64 and p["tiles_y"] * 4 >= H > (p["tiles_y"] - 1) * 4
        assert p["blocks"] == p["tiles_x"] * p["tiles_y"] * B * P


def test_plan_bands_and_refusals(lib):
    from mal_amd import _lib
    # every tile band: widths around one and two tiles, heights around one and two tile rows
    for W, tx in ((2, 1), (63, 1), (64, 1), (65, 2), (128, 2), (129, 3), (512, 8)):
        for H, ty in ((2, 1), (3, 1), (4, 1), (5, 2), (8, 2), (9, 3), (192, 48)):
            p = plan(lib, 2, 3, H, W, 3, 2)
            assert (p["tiles_x"], p["tiles_y"], p["blocks"]) == (tx, ty, tx * ty * 4)
    # the table's cases include a ragged last tile (w65, h5_up4) and a shape that spans two rows of tiles (h5_up4)
    assert plan(lib, 2, 3, 5, 70, 4, 1)["tiles_x"] == 2 and plan(lib, 2, 3, 5, 70, 4, 1)["tiles_y"] == 2
    n = None
    f = lib.mal_forward_warp_plan
    assert f(1, 3, 2, 2, 3, 1, n, n, n, n, n, n, n) == 0  # every output pointer is nullable
    for bad in ((1, 3, 1, 8, 3, 1), (1, 3, 8, 1, 3, 1), (1, 3, 8, 8, 0, 1), (1, 3, 8, 8, 5, 1), (1, 0, 8, 8, 3, 1), (1, 5, 8, 8, 3, 1),
                (1, 3, 8, 8, 3, 0), (1, 3, 8, 8, 3, 5), (0, 3, 8, 8, 3, 1), (4, 4, 16384, 16384, 3, 1), (70000, 1, 2, 2, 1, 1)):
        assert f(*bad, n, n, n, n, n, n, n) == -2, bad
    for B, H, W, P in ((1, 1, 8, 1), (1, 8, 1, 1), (0, 8, 8, 1), (1, 8, 8, 0), (1, 8, 8, 5), (70000, 2, 2, 1), (4, 16384, 16384, 4)):
        assert lib.mal_forward_warp_workspace_bytes(B, H, W, P) == 0
    assert lib.mal_forward_warp_workspace_bytes(12, 192, 512, 2) >= 2 * 12 * 192 * 512 * 4
    assert lib.mal_forward_warp_workspace_bytes(12, 192, 512, 1) < lib.mal_forward_warp_workspace_bytes(12, 192, 512, 2)
    # null pointers are MAL_EINVAL, shapes MAL_ESHAPE, both before any HIP call (there is no device here)
    assert lib.mal_forward_warp(None) == -1
    a = _lib.FwarpArgs()
    assert lib.mal_forward_warp(ctypes.byref(a)) == -1
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    a.img = a.depth = a.K = a.img_w = a.depth_w = a.valid = a.ws = p
    a.pose[0] = p
    a.B, a.C, a.H, a.W, a.upscale, a.n_pose = 1, 3, 1, 8, 3, 1
    assert lib.mal_forward_warp(ctypes.byref(a)) == -2
    a.H, a.upscale = 8, 5
    assert lib.mal_forward_warp(ctypes.byref(a)) == -2
    a.upscale, a.ws_bytes = 3, 16
    assert lib.mal_forward_warp(ctypes.byref(a)) == -3
    assert lib.mal_inverse_warp(n, n, n, n, 1, 3, 8, 8, n, n, n, 0, n) == -1
    assert lib.mal_inverse_warp(p, p, p, p, 1, 3, 1, 8, p, p, p, 1 << 20, n) == -2
    assert lib.mal_inverse_warp(p, p, p, p, 1, 3, 8, 8, p, p, p, 16, n) == -3


def test_host_refusals(lib):
    from mal_amd import _lib, rigid_warp
    img, depth = torch.rand(1, 3, 8, 8), torch.rand(1, 1, 8, 8) + 1
    pose, K = torch.eye(4)[None, :3], torch.eye(3)[None]
    with pytest.raises(_lib.MalError, match="CPU|CUDA"):
        rigid_warp.forward_warp(img, depth, pose, K, upscale=3)
    with pytest.raises(_lib.MalError, match="CPU|CUDA"):
        rigid_warp.inverse_warp(img, depth[:, 0], torch.zeros(1, 6), K)
    with pytest.raises(ValueError, match="upscale"):
        rigid_warp.forward_warp(img, depth, pose, K)
    for shape in ((1, 3, 1, 8), (1, 3, 8, 1)):
        with pytest.raises(_lib.MalError, match="2x2"):
            rigid_warp.forward_warp(torch.rand(shape), torch.rand(shape[0], 1, *shape[2:]), pose, K, upscale=3)
        with pytest.raises(_lib.MalError, match="2x2"):
            rigid_warp.inverse_warp(torch.rand(shape), torch.rand(shape[0], *shape[2:]), torch.zeros(1, 6), K)
    for which in range(4):
        args = [img, depth, pose, K]
        args[which] = args[which].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match=r"trainer\.py:494"):
            rigid_warp.forward_warp(*args, upscale=3)
    with pytest.raises(NotImplementedError, match="quat"):
        rigid_warp.inverse_warp(img, depth[:, 0], torch.zeros(1, 6), K, rotation_mode="quat")
    with pytest.raises(NotImplementedError, match="border"):
        rigid_warp.inverse_warp(img, depth[:, 0], torch.zeros(1, 6), K, padding_mode="border")
    with pytest.raises(NotImplementedError, match=r"trainer\.py:494"):
        rigid_warp.warp_dynamic_objects(img.requires_grad_(True), depth, K, depth, pose, img.clone(), depth)
    # forward_warp takes the two mode arguments and ignores them, as upstream does
    with pytest.raises(_lib.MalError, match="CPU|CUDA"):
        rigid_warp.forward_warp(img.detach(), depth, pose, K, upscale=3, rotation_mode="quat", padding_mode="border")


def test_nothing_under_mal_amd_imports_the_oracle():
    import os
    src = open(os.path.join(os.path.dirname(R.__file__), "..", "mal_amd", "rigid_warp.py")).read()
    assert "oracle" not in src and "tests" not in src.replace("tests/", "")
