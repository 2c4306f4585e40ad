"""GPU: mal_amd.rigid_warp (mal_forward_warp / mal_inverse_warp, mal_amd/csrc/mal_fwarp.hip) against the restatement of
DynamicDepth's forward_warp (tests/fwarp_restated.py, held to the reference bit for bit in fp32 by tests/test_fwarp_cases.py)
evaluated in fp64 on the host.  No test here reads the reference tree.

Splat gate.  The exported z-buffer against the fp64 restatement's: a cell differs when it is off by more than
max(1e-6, 1.25 x the fp32 restatement's own distance) relative; at most 3e-4 N + 8 cells may (N sub-points), and each must
have a near-tie sub-point (x or y within 1e-4 of a truncation edge in fp64) that fp64 puts in it or next to it.
Resolve gate.  The kernel's OWN z-buffer is forced on the restatement's stage 2 in fp64: valid may differ only where
|coord| is within 1e-5 of 1, under the same cap; depth_w within max(1e-5, 1.25 x fp32 distance) relative; img_w within
max(1e-4, 1.25 x fp32 distance) of the image scale -- the floors tests/test_gpu_layers.py uses for depths and warped images.
The identity pose is not a decision case (tests/test_fwarp_cases.py shows why); it is held by properties that need no
tie-breaking.  Measured figures: DESIGN.md."""
import functools

import numpy as np
import pytest
import torch

from mal_amd import ops, rigid_warp
from tests import fwarp_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DECISION_CASES = [k for k in R.GPU_CASES if R.CASES[k][5] != "identity"]
IDENTITY_CASES = [k for k in R.CASES if R.CASES[k][5].startswith("identity") and R.CASES[k][4] >= 2]


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.int32)


def zfloat(zb):
    return zb.cpu().numpy().view(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """the inputs, the fp32 and fp64 splat of the restatement (computed once, never modified) and the kernel's outputs"""
    c = R.make_case(name)
    c["s32"] = R.splat(c["depth"], c["pose"], c["K"], c["up"], torch.float32)
    c["s64"] = R.splat(c["depth"], c["pose"], c["K"], c["up"], torch.float64)
    c["dev"] = {k: c[k].to(DEV) for k in ("img", "depth", "pose", "K")}
    return c


def launch(c, poses=None, **kw):
    d = c["dev"]
    return ops.forward_warp(d["img"], d["depth"][:, 0], [d["pose"]] if poses is None else poses, d["K"], c["up"], want_zbuf=True, **kw)


def as_upstream(out, q=0):
    img_w, depth_w, valid, _ = out
    return {"img_w": img_w[q].cpu().numpy(), "depth_w": depth_w[q].unsqueeze(1).cpu().numpy(), "valid": valid[q].unsqueeze(1).cpu().numpy()}


@pytest.mark.parametrize("name", DECISION_CASES)
def test_splat_and_resolve_gates(name):
    c = case(name)
    B, _, H, W = c["depth"].shape
    N = c["s64"]["cell"].numel()
    out = launch(c)
    z = zfloat(out[3][0])
    assert np.isfinite(z).all() and (z >= 0).all() and (z <= 1000).all()
    n_z, gate = R.check_zbuf(z, c["s32"], c["s64"], H, W)
    zk = torch.from_numpy(z.copy())
    r32 = R.resolve(zk, c["img"], c["pose"], c["K"], torch.float32)
    r64 = R.resolve(zk, c["img"], c["pose"], c["K"], torch.float64)
    rep = R.check_resolve(as_upstream(out), r32, r64, 1.0, N)
    print("%s: z-buffer cells differing %d of %d (gate %.2g, cap %.0f); valid differing %d; depth_w %.2g rel (gate %.2g); img_w %.2g "
          "(gate %.2g)" % (name, n_z, z.size, gate, R.cap(N), rep["valid_diff"], rep["depth_rel"], rep["depth_gate"], rep["img"], rep["img_gate"]))
    # the public function returns upstream's tuple
    d = c["dev"]
    img_w, depth_w, valid = rigid_warp.forward_warp(d["img"], d["depth"], d["pose"], d["K"], upscale=c["up"])
    assert img_w.shape == c["img"].shape and depth_w.shape == c["depth"].shape and valid.shape == c["depth"].shape
    assert np.array_equal(bits(img_w), bits(out[0][0])) and np.array_equal(bits(depth_w[:, 0]), bits(out[1][0]))
    assert np.array_equal(bits(valid[:, 0]), bits(out[2][0]))
    if R.CASES[name][5] == "all_outside":
        for t in out:
            assert not t.any()


@pytest.mark.parametrize("name", ["ref_b3_37x50_s1", "tiny_2x2", "w65", "c4_per_k", "large_motion"])
def test_inverse_warp_gate(name):
    """mal_inverse_warp on the case's own depth map and a 6-vector pose, under the resolve gate"""
    c = case(name)
    B, C, H, W = c["img"].shape
    rng = np.random.default_rng(77)
    k = 5.0 if name == "large_motion" else 1.0
    pose6 = torch.from_numpy(np.concatenate([0.05 * k * rng.standard_normal((B, 3)), 0.01 * k * rng.standard_normal((B, 3))], 1).astype(np.float32))
    depth = c["depth"][:, 0]
    o32, v32, _ = R.inverse_warp(c["img"], depth, pose6, c["K"], torch.float32)
    o64, v64, co = R.inverse_warp(c["img"], depth, pose6, c["K"], torch.float64)
    out, valid = rigid_warp.inverse_warp(c["dev"]["img"], c["dev"]["depth"][:, 0], pose6.to(DEV), c["dev"]["K"])
    assert valid.dtype == torch.bool and valid.shape == (B, H, W) and out.shape == (B, C, H, W)
    dv = valid.cpu().numpy() != v64.numpy()
    tie = np.abs(np.abs(co.numpy()).max(-1) - 1) <= R.COORD_TOL
    assert dv.sum() <= R.cap(B * H * W) and not (dv & ~tie).any()
    own = float((o32.double() - o64).abs().max())
    got = float((out.cpu().double() - o64).abs().max())
    print("%s: inverse warp %.2g of the image scale (fp32 restatement %.2g), %d valid flags differ" % (name, got, own, dv.sum()))
    assert got <= max(1e-4, 1.25 * own)


@pytest.mark.parametrize("name", IDENTITY_CASES)
def test_identity_pose_properties(name):
    """no holes (for upscale >= 2: the sub-points strictly inside a pixel stay inside it; at upscale 1 the only sub-point
    sits on the lattice and the reference itself leaves holes); every cell holds at least its own pixel's 1/Z and at most
    the largest of its 3x3 neighbourhood, at 1 ulp"""
    c = case(name)
    out = launch(c)
    zb = out[3][0].cpu().numpy()
    assert (zb != 0).all()
    own = (np.float32(1) / np.maximum(c["depth"][:, 0].numpy(), np.float32(1e-3))).view(np.int32)
    assert (zb >= own - 1).all()
    pad = np.pad(own, ((0, 0), (1, 1), (1, 1)), mode="edge")
    H, W = own.shape[1:]
    hood = np.max([pad[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], 0)
    assert (zb <= hood + 1).all()
    assert (out[2][0] == 1).float().mean() > 0.9


@pytest.mark.parametrize("name", ["ref_b2_24x72_s0", "h5_up4", "converge"])
def test_repeatable_and_no_stale_zbuffer(name):
    c = case(name)
    first = [bits(t) for t in launch(c)]
    again = [bits(t) for t in launch(c)]
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    # the same workspace then holds another input's buffer (nearer depths everywhere: every cell's maximum is larger)
    d = c["dev"]
    other = ops.forward_warp(d["img"], d["depth"][:, 0] * 0.25, [d["pose"]], d["K"], c["up"], want_zbuf=True)
    assert not np.array_equal(bits(other[3]), first[3])
    third = [bits(t) for t in launch(c)]
    for a, b in zip(first, third):
        assert np.array_equal(a, b)


def second_pose(c):
    p = c["pose"].clone()
    p[:, :, 3] = -p[:, :, 3]
    p[:, :3, :3] = p[:, :3, :3].transpose(1, 2)
    return p.contiguous().to(DEV)


@pytest.mark.parametrize("name", ["ref_b3_37x50_s0", "w65"])
def test_two_poses_in_one_call_equal_two_calls(name):
    c = case(name)
    p0, p1 = c["dev"]["pose"], second_pose(c)
    both = launch(c, [p0, p1])
    for q, p in enumerate((p0, p1)):
        one = launch(c, [p])
        for a, b in zip(both, one):
            assert a.shape[0] == 2 and np.array_equal(bits(a[q]), bits(b[0]))
    assert not np.array_equal(bits(both[3][0]), bits(both[3][1]))


def composition_inputs(c, seed=5):
    B, C, H, W = c["img"].shape
    g = torch.Generator().manual_seed(seed)
    dst = torch.rand(B, C, H, W, generator=g) + 0.25
    mask = (torch.rand(B, 1, H, W, generator=g) < 0.4).float()
    return dst, mask


@pytest.mark.parametrize("no_reproj", [False, True])
@pytest.mark.parametrize("name", ["ref_b3_37x50_s2", "c4_per_k"])
def test_composition_is_upstreams_index_assignment(name, no_reproj):
    """trainer.py:506-510 done in torch on the kernel's own img_w; per element and per channel: channel 0 of the image is
    zeroed on the left half, so img_w > 0 holds for some channels of a pixel and not for others"""
    c = case(name)
    B, C, H, W = c["img"].shape
    img = c["img"].clone()
    img[:, 0, :, :W // 2] = 0
    dst, mask = composition_inputs(c)
    d = c["dev"]
    dst_dev = dst.to(DEV)
    img_w, _, _, _ = ops.forward_warp(img.to(DEV), d["depth"][:, 0], [d["pose"]], d["K"], c["up"], dst=[dst_dev],
                                      masks=[(mask[:, 0] == 1).to(DEV)], no_reproj=no_reproj)
    w = img_w[0].cpu()
    want = R.compose(dst, w, mask, no_reproj)
    assert np.array_equal(bits(dst_dev), bits(want))
    some = (w > 0).any(1) & ~(w > 0).all(1)
    assert some.any(), "no pixel with img_w > 0 on some channels only: the case does not show per-channel composition"
    assert not np.array_equal(bits(want), bits(dst))
    # without a mask only the pasted elements change
    dst2 = dst.to(DEV)
    ops.forward_warp(img.to(DEV), d["depth"][:, 0], [d["pose"]], d["K"], c["up"], dst=[dst2], no_reproj=no_reproj)
    assert np.array_equal(bits(dst2), bits(R.compose(dst, w, None, no_reproj)))


def test_warp_dynamic_objects_mirrors_the_trainer():
    """trainer.py:493-534 in two library calls against the same steps in torch on the kernel's own warps; deselected
    samples of the lookup frame are untouched to the bit"""
    c = case("ref_b3_37x50_s3")
    B, C, H, W = c["img"].shape
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.rand(*s, generator=g)
    doj, doj_m1, doj_p1 = [(rnd(B, 1, H, W) < 0.5).float() for _ in range(3)]
    color_m1, color_p1, lookup, color_aug = rnd(B, C, H, W) + 0.1, rnd(B, C, H, W) + 0.1, rnd(B, C, H, W) + 0.1, rnd(B, C, H, W)
    aug = torch.zeros(B, 1, H, W)
    aug[1] = 1  # sample 1 had a cost-volume augmentation: its lookup frame stays
    d = c["dev"]
    p1 = second_pose(c)
    for no_reproj, no_teacher in ((False, False), (True, True)):
        cm1, cp1, lk = color_m1.to(DEV), color_p1.to(DEV), lookup.to(DEV)
        out = rigid_warp.warp_dynamic_objects(d["img"], d["depth"], d["K"], doj.to(DEV), d["pose"], cm1, doj_m1.to(DEV), pose_p1=p1,
                                              color_p1=cp1, doj_mask_p1=doj_p1.to(DEV), color_aug=color_aug.to(DEV), lookup_frame=lk,
                                              augmentation_mask=aug.to(DEV), upscale=c["up"], no_reproj_doj=no_reproj,
                                              no_teacher_warp=no_teacher)
        tgt = (c["img"] * (doj != 0).float()).to(DEV)
        w_m1, _, _ = rigid_warp.forward_warp(tgt, d["depth"], d["pose"], d["K"], upscale=c["up"])
        w_p1, _, _ = rigid_warp.forward_warp(tgt, d["depth"], p1, d["K"], upscale=c["up"])
        w_aug, _, _ = rigid_warp.forward_warp((color_aug * (doj != 0).float()).to(DEV), d["depth"], d["pose"], d["K"], upscale=c["up"])
        assert np.array_equal(bits(out["img_w_m1"]), bits(w_m1)) and np.array_equal(bits(out["img_w_p1"]), bits(w_p1))
        assert np.array_equal(bits(out["imgaug_w_m1"]), bits(w_aug))
        assert np.array_equal(bits(cm1), bits(R.compose(color_m1, w_m1.cpu(), doj_m1, no_reproj)))
        assert np.array_equal(bits(cp1), bits(R.compose(color_p1, w_p1.cpu(), doj_p1, no_reproj)))
        want = R.compose(lookup, w_aug.cpu(), doj_m1, False)  # :519-520 paste the warp whatever no_reproj_doj says
        want[1] = lookup[1]
        assert np.array_equal(bits(lk), bits(want))
        assert np.array_equal(bits(lk[1]), bits(lookup[1])) and not np.array_equal(bits(lk[0]), bits(lookup[0]))
        if no_teacher:
            assert np.array_equal(bits(out["ori_color_m1"]), bits(color_m1)) and np.array_equal(bits(out["ori_color_p1"]), bits(cm1))
        else:
            assert "ori_color_m1" not in out


def test_graph_capture_and_device_side_selector():
    """forward_warp is capturable (no allocation inside the library, no readback); the captured composition follows a
    selector and inputs rewritten between replays"""
    c = case("ref_b2_24x72_s0")
    B, C, H, W = c["img"].shape
    d = c["dev"]
    dst0, mask = composition_inputs(c)
    depth = d["depth"].clone()
    dst, sel = dst0.to(DEV), torch.ones(B, dtype=torch.uint8, device=DEV)
    m = (mask[:, 0] == 1).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.forward_warp(d["img"], depth[:, 0], [d["pose"]], d["K"], c["up"], dst=[dst.clone()], masks=[m], select=sel)  # warm: workspace
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            img_w, depth_w, valid = rigid_warp.forward_warp(d["img"], depth, d["pose"], d["K"], upscale=c["up"])
            comp = ops.forward_warp(d["img"], depth[:, 0], [d["pose"]], d["K"], c["up"], dst=[dst], masks=[m], select=sel)
    torch.cuda.current_stream().wait_stream(s)
    for new_depth, selector in ((d["depth"], [1, 1]), (d["depth"] * 0.5, [0, 1]), (d["depth"], [1, 0])):
        depth.copy_(new_depth)
        dst.copy_(dst0)
        sel.copy_(torch.tensor(selector, dtype=torch.uint8))
        graph.replay()
        torch.cuda.synchronize()
        e_img, e_depth, e_valid = rigid_warp.forward_warp(d["img"], new_depth.contiguous(), d["pose"], d["K"], upscale=c["up"])
        assert np.array_equal(bits(img_w), bits(e_img)) and np.array_equal(bits(depth_w), bits(e_depth))
        assert np.array_equal(bits(valid), bits(e_valid)) and np.array_equal(bits(comp[0][0]), bits(e_img))
        want = R.compose(dst0, e_img.cpu(), mask)
        for b in range(B):
            if not selector[b]:
                want[b] = dst0[b]
        assert np.array_equal(bits(dst), bits(want))


def test_nan_and_inf_depths_contribute_nothing():
    """poisoned source pixels land nowhere: the z-buffer can only lose their contributions (<= the clean one everywhere,
    EQUAL outside the 3x3 surroundings of the cells fp64 sends their sub-points to), and nothing non-finite comes out"""
    c = case("ref_b3_37x50_s0")
    B, _, H, W = c["depth"].shape
    up = c["up"]
    clean = launch(c)
    depth = c["depth"].clone()
    poison = [(0, 3, 4, float("nan")), (0, 20, 41, float("inf")), (1, 0, 0, float("-inf")), (2, 36, 49, float("nan")), (2, 10, 10, float("inf"))]
    touched = np.zeros((B, H + 2, W + 2), bool)
    cell = c["s64"]["cell"].reshape(B, H * up, W * up).numpy()
    for b, y, x, v in poison:
        depth[b, 0, y, x] = v
        for k in cell[b, y * up:(y + 1) * up, x * up:(x + 1) * up].ravel():
            if k >= 0:
                touched[b, k // W:k // W + 3, k % W:k % W + 3] = True
    touched = touched[:, 1:-1, 1:-1]
    d = c["dev"]
    out = ops.forward_warp(d["img"], depth[:, 0].to(DEV), [d["pose"]], d["K"], up, want_zbuf=True)
    for t in out[:3]:
        assert torch.isfinite(t).all()
    zc, zp = clean[3][0].cpu().numpy(), out[3][0].cpu().numpy()
    assert (zp <= zc).all() and np.array_equal(zp[~touched], zc[~touched])
    assert 0 < touched.mean() < 0.2
    # and the restatement, which applies the same float range test, agrees under the splat gate
    s32 = R.splat(depth, c["pose"], c["K"], up, torch.float32)
    s64 = R.splat(depth, c["pose"], c["K"], up, torch.float64)
    R.check_zbuf(zfloat(out[3][0]), s32, s64, H, W)
    # stage 2 reads only the z-buffer: where it is unchanged (and its 2x2 sampling footprint cannot matter, depth_w being
    # per pixel), the outputs are unchanged to the bit
    same = torch.from_numpy(zp == zc).to(DEV)
    assert torch.equal(out[1][0][same], clean[1][0][same]) and torch.equal(out[2][0][same], clean[2][0][same])
    assert torch.equal(out[0][0][same[:, None].expand_as(out[0][0])], clean[0][0][same[:, None].expand_as(out[0][0])])


def test_refusals_on_the_device():
    c = case("tiny_2x2")
    d = c["dev"]
    from mal_amd import _lib
    with pytest.raises(_lib.MalError, match="shape"):
        ops.forward_warp(d["img"], d["depth"][:, 0], [d["pose"]], d["K"], 5)
    with pytest.raises(_lib.MalError):
        ops.forward_warp(d["img"], d["depth"][:, 0], [d["pose"]] * 5, d["K"], 3)
    with pytest.raises(_lib.MalError, match="float32"):
        ops.forward_warp(d["img"].double(), d["depth"][:, 0], [d["pose"]], d["K"], 3)
