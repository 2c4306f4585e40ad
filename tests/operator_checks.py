"""What the operator sweep shares (tests/test_operator_cases.py on the CPU, tests/test_gpu_operator_sweep.py on the device):
the case tables, the input builders, the float64 / float32 references and the gate.

The operator layer is mal_amd/ops.py over csrc/mal_warp.hip, mal_photo.hip, mal_photo_march.hip and mal_pose.hip.  The gate is
``tests.epipolar_checks.check`` unchanged: a device tensor is held within ``max(floor, 1.25 x the float32 torch reference's own
distance from float64)`` of the float64 reference, relative to the tensor's scale; forward values and sums of few elements on
every element, per-pixel gradient maps with the allowance ``2e-4 + 4/numel``.  ``floor`` is what tests/test_gpu_layers.py
asserts for the same operator.  A case is admissible when the float32 reference alone passes at the floor
(``epipolar_checks.admissible``'s form, ``ref32=None``); a case that does not gets the next seed (``seed`` in its options).

Where an operator decides something discontinuous both sides evaluate the same smooth function:
* bilinear taps / border clip: the kernel's own taps (``aten_restated.taps_of`` on the float32 grid) are forced on
  ``grid_sample_forced_taps``; lattice grids (coordinates exact in float32 and float64) use torch's sampler as it is;
* SSIM's clamp: values everywhere; gradients exempt where the float64 pre-clamp value is within 1e-5 of 0 or 1;
* |a - b| of float32 inputs: the sign is exact, ties are zero as ``torch.abs``'s gradient, nothing is exempt;
* min over candidates / automask / the epilogue's winner: the device's decisions are forced on the reference and may differ
  from the float64 reference's own at no more than ``3e-4 N + 8`` pixels, each a near-tie (gap <= 1e-4)."""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import aten_restated as AR
from oracle import mal_oracle as O
from tests.epipolar_checks import check, distance  # noqa: F401  (the gate, unchanged)

DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
EPS24 = 2.0 ** -24
PX_PER_BLOCK = 1024        # kPxPerBlock: pixels per workgroup of warp_bwd / project3d_bwd
F_AUTOMASK, F_NO_SSIM, F_AVG, F_DUAL_DISTIL = 1, 8, 16, 64


def seed_of(name, extra=0):
    return zlib.crc32(name.encode()) % 10000 + extra


def gen(name, extra=0):
    return torch.Generator().manual_seed(seed_of(name, extra))


def ew_blocks(n, cap):
    """workgroups of a capped grid-stride launch, and whether a thread makes more than one trip"""
    g = min(max((n + 255) // 256, 1), cap)
    return g, n > cap * 256


def decision_cap(n):
    return 3e-4 * n + 8


def hold_decisions(dev, ref, gap, what, tie=1e-4):
    """``dev`` and ``ref`` decision maps; ``gap``: the float64 margin of the decision per pixel.  -> number of differences"""
    diff = dev != ref
    n = int(diff.sum())
    assert n <= decision_cap(diff.numel()), (what, n, diff.numel())
    if n:
        assert float(gap[diff].abs().max()) <= tie, (what, float(gap[diff].abs().max()))
    return n


# ================================================================ 1. elementwise geometry
FLAT_N = {"n1": 1, "n255": 255, "n257": 257, "n589824_past_2048_blocks": 3 * 384 * 512}
# back-projection and texel packing refuse H or W below 2: 258 = 2 x 129 straddles the 256-thread block instead of 257
PLANE_SHAPES = {"b1_2x2": (1, 2, 2), "b1_15x17_n255": (1, 15, 17), "b1_2x129_n258": (1, 2, 129),
                "b3_384x512_past_2048_blocks": (3, 384, 512)}
DEPTH_RANGES = ((0.1, 100.0), (0.5, 80.0))


def per_sample_K(B, H, W, g, jitter=0.05):
    from mal_amd.synthetic import kitti_intrinsics
    K = kitti_intrinsics(B, H, W)[0].clone()
    K[:, 0, 0] *= 1 + jitter * (2 * torch.rand(B, generator=g) - 1)
    K[:, 1, 1] *= 1 + jitter * (2 * torch.rand(B, generator=g) - 1)
    K[:, 0, 2] += jitter * W * (2 * torch.rand(B, generator=g) - 1)
    K[:, 1, 2] += jitter * H * (2 * torch.rand(B, generator=g) - 1)
    return K.contiguous(), torch.linalg.inv(K.double()).float().contiguous()


def flat_case(name):
    n, g = FLAT_N[name], gen(name)
    disp = torch.sigmoid(1.5 * torch.randn(n, generator=g) - 1.0)
    mono = 0.5 + 20 * torch.rand(n, generator=g)
    lowest = (1 / mono) * torch.exp(0.6 * torch.randn(n, generator=g))
    k = min(n, 4)
    lowest[:k] = torch.tensor([0.0, 1e30, 3.0, 0.5])[:k]          # 1/0 = inf: mask 0; a huge cost: mask 0
    return dict(disp=disp, g_scaled=torch.randn(n, generator=g), g_depth=torch.randn(n, generator=g), mono=mono,
                lowest=lowest, cmask=(torch.rand(n, generator=g) < 0.8).float())


def ref_disp_to_depth(c, dtype, lo, hi, use=("g_scaled", "g_depth")):
    d = c["disp"].to(dtype).clone().requires_grad_(True)
    scaled, depth = O.disp_to_depth(d, lo, hi)
    s = sum((o * c[k].to(dtype)).sum() for o, k in ((scaled, "g_scaled"), (depth, "g_depth")) if k in use)
    s.backward()
    return dict(scaled=scaled.detach(), depth=depth.detach()), dict(g_disp=d.grad)


def ref_matching_mask(c, dtype, with_cmask=True):
    """-> the mask and the two ratios' distances from the threshold 1 (float64: the margin of each decision)"""
    mono, lc = c["mono"].to(dtype).reshape(1, 1, 1, -1), c["lowest"].to(dtype).reshape(1, 1, -1)
    m = O.compute_matching_mask({("mono_depth", 0, 0): mono, "lowest_cost": lc}).to(dtype).reshape(-1)
    matching = 1 / lc.reshape(-1)
    r1, r2 = (matching - mono.reshape(-1)) / mono.reshape(-1), (mono.reshape(-1) - matching) / matching
    gap = torch.minimum((r1 - 1).abs(), (r2 - 1).abs())
    return (m * c["cmask"].to(dtype) if with_cmask else m), torch.nan_to_num(gap, nan=1e30, posinf=1e30)


def plane_case(name):
    B, H, W = PLANE_SHAPES[name]
    g = gen(name)
    K, inv_K = per_sample_K(B, H, W, g)
    return dict(depth=0.5 + 20 * torch.rand(B, 1, H, W, generator=g), K=K, inv_K=inv_K,
                g_points=torch.randn(B, 4, H * W, generator=g), img=torch.rand(B, 3, H, W, generator=g))


def ref_backproject(c, dtype):
    d = c["depth"].to(dtype).clone().requires_grad_(True)
    pts = O.backproject_depth(d, c["inv_K"].to(dtype))
    (pts * c["g_points"].to(dtype)).sum().backward()
    return dict(points=pts.detach()), dict(g_depth=d.grad)


# ================================================================ 2. project3d, warp
# name: (B, H, W, convention, F, options).  bps = ceil(HW / 1024) walks tail_pose_block's stride-10 loop and its unroll by 8
WARP_CASES = {
    "bps1_2x2": (1, 2, 2, 0, 1, {}),
    "bps1_19x33_dualrefine": (2, 19, 33, 1, 2, {}),
    "bps2_33x32": (1, 33, 32, 0, 2, dict(need_T=(False, True))),
    "bps9_72x120_dualrefine": (1, 72, 120, 1, 1, {}),
    "bps10_96x100_b3_per_sample_K": (3, 96, 100, 0, 2, dict(need_T=(True, False))),
    "bps11_96x110": (1, 96, 110, 1, 2, {}),
    "bps21_128x164": (1, 128, 164, 0, 1, {}),
    "bps81_192x432": (1, 192, 432, 0, 2, {}),
    "third_behind_the_camera_24x40": (2, 24, 40, 0, 1, dict(behind=True)),
}
BPS_WANTED = {1, 2, 9, 10, 11, 21, 81}


def bps_of(H, W):
    return (H * W + PX_PER_BLOCK - 1) // PX_PER_BLOCK


def warp_case(name):
    from mal_amd.synthetic import make_batch
    B, H, W, conv, Fr, opts = WARP_CASES[name]
    g = gen(name, opts.get("seed", 0))
    b = make_batch(B, H, W, seed=seed_of(name, opts.get("seed", 0)))
    K, inv_K = per_sample_K(B, H, W, g)
    Ts = [O.transformation_from_parameters(b["axisangle_m1"], b["translation_m1"], True),
          O.transformation_from_parameters(b["axisangle_p1"], b["translation_p1"], False)][:Fr]
    disp = b["disp_teacher"]
    if opts.get("behind"):  # depths are 0.1 .. 100 with a median of a few units: pull a third of the points behind the camera
        depth = O.disp_to_depth(disp, 0.1, 100.0)[1]
        q = torch.quantile(depth.flatten(1), 1.0 / 3, dim=1).view(B, 1, 1, 1)
        # ... and keep every |z| above a tenth of the depth: the relative error of z = depth - q is float32's times depth/|z|,
        # and the pixel nearest z = 0 sets the grid's scale
        depth = torch.where((depth / q - 1).abs() < 0.1, torch.where(depth < q, 0.9 * q, 1.1 * q), depth)
        disp = ((1 / depth - 0.01) / 9.99).contiguous()
        Ts = [T.clone() for T in Ts]
        for T in Ts:
            T[:, :3, :3], T[:, :3, 3] = torch.eye(3), 0.0
            T[:, 2, 3] = -q.view(B)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(disp=disp, K=K, inv_K=inv_K, Ts=[T.contiguous() for T in Ts], srcs=[b["color_m1"], b["color_p1"]][:Fr],
                g_warped=[rn(B, 3, H, W) for _ in range(Fr)], g_grid=[rn(B, H, W, 2) for _ in range(Fr)],
                g_depth=rn(B, 1, H, W), g_z=rn(B, 1, H, W), conv=conv, need_T=opts.get("need_T", (True,) * Fr),
                behind=bool(opts.get("behind")))


def _conv(c):
    return "manydepth" if c["conv"] == 0 else "dualrefine"


def ref_warp(c, dtype, taps=None, use=("g_warped", "g_grid", "g_depth")):
    """depth, grids (and warped images under the forced ``taps`` per frame) and the gradients of the cotangents in ``use``"""
    B, _, H, W = c["disp"].shape
    d = c["disp"].to(dtype).clone().requires_grad_(True)
    Ts = [T.to(dtype).clone().requires_grad_(True) for T in c["Ts"]]
    depth = O.disp_to_depth(d, 0.1, 100.0)[1]
    pts = O.backproject_depth(depth, c["inv_K"].to(dtype))
    out, s = dict(depth=depth.detach()), 0
    if "g_depth" in use:
        s = s + (depth * c["g_depth"].to(dtype)).sum()
    for f, T in enumerate(Ts):
        grid = O.project_3d(pts, c["K"].to(dtype), T, H, W, convention=_conv(c))
        out["grid%d" % f] = grid.detach()
        if "g_grid" in use:
            s = s + (grid * c["g_grid"][f].to(dtype)).sum()
        if taps is not None:
            x0, y0, cx, cy = taps[f]
            wp = AR.grid_sample_forced_taps(c["srcs"][f].to(dtype), grid, x0, y0, cx, cy, align_corners=c["conv"] == 0)
            out["warped%d" % f] = wp.detach()
            if "g_warped" in use:
                s = s + (wp * c["g_warped"][f].to(dtype)).sum()
    s.backward()
    grads = dict(g_disp=d.grad)
    for f, T in enumerate(Ts):
        grads["g_T%d" % f] = T.grad if c["need_T"][f] else None
    return out, grads


def ref_project(c, points, dtype, want_z=True, use_gz=True):
    B, _, H, W = c["disp"].shape
    p = points.to(dtype).clone().requires_grad_(True)
    T = c["Ts"][0].to(dtype).clone().requires_grad_(True)
    grid, z = O.project_3d(p, c["K"].to(dtype), T, H, W, convention=_conv(c), with_depth=True)
    s = (grid * c["g_grid"][0].to(dtype)).sum()
    if use_gz:
        s = s + (z * c["g_z"].to(dtype)).sum()
    s.backward()
    out = dict(grid=grid.detach())
    if want_z:
        out["z"] = z.detach()
    return out, dict(g_points=p.grad, g_T=T.grad)


# ================================================================ 3. grid_sample
# name: (B, C, H, W, Ho, Wo, align_corners, kind)
GRID_CASES = {
    "c1_5x9_to_7x3": (2, 1, 5, 9, 7, 3, True, "random"),
    "c3_5x9_to_1x1_dualrefine": (2, 3, 5, 9, 1, 1, False, "random"),
    "c5_6x1_source_one_column": (1, 5, 6, 1, 4, 5, True, "random"),
    "c3_1x7_source_one_row_dualrefine": (1, 3, 1, 7, 4, 5, False, "random"),
    "c5_17x33_dualrefine": (2, 5, 17, 33, 17, 33, False, "random"),
    "c1_5x9_to_600x900_past_2048_blocks": (1, 1, 5, 9, 600, 900, True, "random"),
    "lattice_ac_3x2": (1, 3, 3, 2, 0, 0, True, "lattice"),
    "lattice_ac_5x9": (2, 1, 5, 9, 0, 0, True, "lattice"),
    "lattice_ac_17x3": (1, 5, 17, 3, 0, 0, True, "lattice"),
    "lattice_dualrefine_1x2": (1, 3, 1, 2, 0, 0, False, "lattice"),
    "lattice_dualrefine_4x8": (2, 1, 4, 8, 0, 0, False, "lattice"),
    "lattice_dualrefine_16x2": (1, 5, 16, 2, 0, 0, False, "lattice"),
}
LATTICE_SIZES = {1, 2, 4, 8, 16}


def lattice(size, ac):
    """normalised coordinates that unnormalise EXACTLY (float32 and float64) to k = -1 .. size"""
    k = torch.arange(-1, size + 1, dtype=F64)
    return 2 * k / (size - 1) - 1 if ac else (2 * k + 1) / size - 1


def grid_case(name):
    B, C, H, W, Ho, Wo, ac, kind = GRID_CASES[name]
    g = gen(name)
    src = torch.rand(B, C, H, W, generator=g)
    if kind == "lattice":
        gx, gy = lattice(W, ac), lattice(H, ac)
        Ho, Wo = gy.numel(), gx.numel()
        grid = torch.stack([gx[None, :].expand(Ho, Wo), gy[:, None].expand(Ho, Wo)], -1)[None].expand(B, Ho, Wo, 2)
        assert torch.equal(grid.float().double(), grid)
        grid = grid.float().contiguous()
        cot = (0.5 + torch.rand(B, C, Ho, Wo, generator=g)) * torch.where(torch.rand(B, C, Ho, Wo, generator=g) < 0.5, -1.0, 1.0)
    else:
        grid = 3.0 * torch.rand(B, Ho, Wo, 2, generator=g) - 1.5      # 1.5 x beyond both borders
        cot = torch.randn(B, C, Ho, Wo, generator=g)
    return dict(src=src, grid=grid, cot=cot, ac=ac, kind=kind)


def ref_grid_sample(c, dtype):
    src, grid = c["src"].to(dtype), c["grid"].to(dtype).clone().requires_grad_(True)
    if c["kind"] == "lattice":
        out = F.grid_sample(src, grid, mode="bilinear", padding_mode="border", align_corners=c["ac"])
    else:  # the kernel's taps: ATen's float32 unnormalisation of the float32 grid
        x0, y0, cx, cy = AR.taps_of(c["grid"], src.shape[2], src.shape[3], align_corners=c["ac"])
        out = AR.grid_sample_forced_taps(src, grid, x0, y0, cx, cy, align_corners=c["ac"])
    (out * c["cot"].to(dtype)).sum().backward()
    return dict(out=out.detach()), dict(g_grid=grid.grad)


def lattice_clipped(c):
    """(B,Ho,Wo,2) bool: positions at or beyond a border, where d/d grid is exactly zero"""
    B, C, H, W = c["src"].shape
    out = torch.zeros(c["grid"].shape, dtype=torch.bool)
    for ax, size in ((0, W), (1, H)):
        i = AR.unnormalize(c["grid"][..., ax].double(), size, c["ac"])
        out[..., ax] = (i <= 0) | (i >= size - 1)
    return out


# ================================================================ 4. ssim, reprojection loss
# name: (B, C, H, W, options)
SSIM_CASES = {
    "c1_2x2": (1, 1, 2, 2, {}),
    "c3_2x7": (2, 3, 2, 7, {}),
    "c3_3x3": (1, 3, 3, 3, {}),
    "c2_3x2": (2, 2, 3, 2, {}),
    "c2_5x130": (3, 2, 5, 130, {}),
    "c3_17x64_zero_cotangent_block": (2, 3, 17, 64, dict(zero_block=True)),
    "c4_17x64": (1, 4, 17, 64, {}),
    "c3_17x64_static_block_x_equals_y": (1, 3, 17, 64, dict(static=(4, 11, 10, 40))),
    "c3_b4_192x512_past_4096_blocks": (4, 3, 192, 512, {}),
}
REPROJ_FORWARD_ONLY = {"c3_b6_384x512_past_4096_blocks": (6, 3, 384, 512, {})}
SMALL_SSIM = ("c1_2x2", "c3_2x7", "c3_3x3", "c2_3x2", "c4_17x64")


def ssim_case(name):
    B, C, H, W, opts = dict(SSIM_CASES, **REPROJ_FORWARD_ONLY)[name]
    g = gen(name, opts.get("seed", 0))
    x = torch.rand(B, C, H, W, generator=g)
    y = (x + 0.1 * torch.randn(B, C, H, W, generator=g)).clamp(0, 1)
    k = min(3, H * W)
    y.view(B, C, -1)[:, :, :k] = x.view(B, C, -1)[:, :, :k]            # exact ties of the L1 term
    cot, cot1 = torch.randn(B, C, H, W, generator=g), torch.randn(B, 1, H, W, generator=g)
    near = torch.zeros(B, C, H, W, dtype=torch.bool)
    if opts.get("zero_block"):
        cot[:, :, 3:9, 5:30], cot1[:, :, 3:9, 5:30] = 0.0, 0.0
    if "static" in opts:
        y0, y1, x0, x1 = opts["static"]
        y[:, :, y0:y1, x0:x1] = x[:, :, y0:y1, x0:x1]
        near[:, :, y0 - 1:y1 + 1, x0 - 1:x1 + 1] = True               # gradients within one pixel of the block: exempt
    return dict(x=x, y=y, cot=cot, cot1=cot1, near=near, static=opts.get("static"))


def ssim_preclamp(x, y):
    """(1 - n/d)/2 of ``mal_oracle.ssim`` before its clamp"""
    pool = lambda t: F.avg_pool2d(F.pad(t, (1, 1, 1, 1), mode="reflect"), 3, 1)
    mu_x, mu_y = pool(x), pool(y)
    sx, sy, sxy = pool(x * x) - mu_x ** 2, pool(y * y) - mu_y ** 2, pool(x * y) - mu_x * mu_y
    n = (2 * mu_x * mu_y + O.SSIM_C1) * (2 * sxy + O.SSIM_C2)
    return (1 - n / ((mu_x ** 2 + mu_y ** 2 + O.SSIM_C1) * (sx + sy + O.SSIM_C2))) / 2


def ssim_exempt(c):
    """pixels whose SSIM gradient is not compared: a window within 1e-5 of the clamp feeds them (float64)"""
    p = ssim_preclamp(c["x"].double(), c["y"].double())
    at = ((p.abs() <= 1e-5) | ((p - 1).abs() <= 1e-5)).double()
    if c["static"] is None:
        return F.max_pool2d(F.pad(at, (1, 1, 1, 1), mode="reflect"), 3, 1) > 0 if at.any() else at.bool()
    return c["near"]


def ref_ssim(c, dtype, reproj=False, no_ssim=False):
    x, y = c["x"].to(dtype).clone().requires_grad_(True), c["y"].to(dtype).clone().requires_grad_(True)
    if reproj:
        out = O.compute_reprojection_loss(x, y, no_ssim=no_ssim)
        (out * c["cot1"].to(dtype)).sum().backward()
    else:
        out = O.ssim(x, y)
        (out * c["cot"].to(dtype)).sum().backward()
    return dict(out=out.detach()), dict(g_x=x.grad, g_y=y.grad)


def masked(grads, exempt):
    return {k: (None if v is None else torch.where(exempt, torch.zeros_like(v), v)) for k, v in grads.items()}


# ================================================================ 5. photo_fwd / photo_bwd
# name: (B, H, W, n_cand, flags, options)
PHOTO_CASES = {
    "n1_2x2": (1, 2, 2, 1, 0, {}),
    "n2_7x59_automask": (3, 7, 59, 2, F_AUTOMASK, dict(ident=True, noise=True, ext=True)),
    "n2_8x60_second_of_the_pair_only": (1, 8, 60, 2, 0, dict(need=(False, True), ext=True)),
    "n2_9x61_automask_no_noise": (1, 9, 61, 2, F_AUTOMASK, dict(ident=True)),
    "n3_17x62_automask": (3, 17, 62, 3, F_AUTOMASK, dict(ident=True, noise=True)),
    "n4_9x63_automask_ties": (1, 9, 63, 4, F_AUTOMASK, dict(ident=True, noise=True, ext=True, need=(True, False, False, True))),
    "n2_17x121_avg": (1, 17, 121, 2, F_AVG, dict(ext=True)),
    "n2_8x125_no_ssim_automask": (3, 8, 125, 2, F_NO_SSIM | F_AUTOMASK, dict(ident=True, noise=True)),
    "n2_17x125_without_min": (1, 17, 125, 2, F_AUTOMASK, dict(ident=True, want=(False, True, True))),
    "n1_9x62_without_argmin": (1, 9, 62, 1, 0, dict(want=(True, False, True), ext=True)),
    "n2_2x121_without_weight": (1, 2, 121, 2, 0, dict(want=(True, True, False))),
    "cus1_rows_grow_2x40x130": (2, 40, 130, 2, F_AUTOMASK, dict(ident=True, noise=True, cus1=True)),
    "cus1_rows_end_at_H_3x9x130": (3, 9, 130, 2, F_AUTOMASK, dict(ident=True, ext=True, cus1=True)),
}
PHOTO_BIG = {"pixel_route_b3_384x512_past_2048_blocks": (3, 384, 512, 1, 0, dict(ext=True, pixel_only=True))}


def march_tasks(B, H, W, cw, cap, rows=8):
    """``decompose`` of mal_photo_march.hip -> (strips, rows, tasks)"""
    strips = (W + cw - 1) // cw
    while rows < H and B * strips * ((H + rows - 1) // rows) > cap:
        rows += 1
    return strips, rows, B * strips * ((H + rows - 1) // rows)


def photo_case(name):
    from mal_amd.synthetic import make_batch
    B, H, W, n, flags, opts = dict(PHOTO_CASES, **PHOTO_BIG)[name]
    g = gen(name, opts.get("seed", 0))
    b = make_batch(B, H, W, seed=seed_of(name, opts.get("seed", 0)))
    cands = [(b["color_m1"] if i % 2 == 0 else b["color_p1"]).clone() for i in range(n)]
    cands = [(c + 0.02 * i * torch.rand(c.shape, generator=g)).clamp(0, 1).contiguous() for i, c in enumerate(cands)]
    tie = None
    if n >= 2 and H >= 7:  # candidate 1 a bit-copy of candidate 0 on a block: the first minimum wins
        tie = (1, min(H, 8), 2, min(W, 40))
        cands[1][:, :, tie[0]:tie[1], tie[2]:tie[3]] = cands[0][:, :, tie[0]:tie[1], tie[2]:tie[3]]
    return dict(target=b["color0"], cands=cands, flags=flags, tie=tie,
                ident=(0.25 * torch.rand(B, 1, H, W, generator=g)) if opts.get("ident") else None,
                noise=torch.randn(B, 1, H, W, generator=g) if opts.get("noise") else None,
                ext=(torch.rand(B, 1, H, W, generator=g) > 0.2).float() if opts.get("ext") else None,
                need=opts.get("need", (True,) * n), want=opts.get("want", (True, True, True)),
                scale=torch.tensor([0.7]), cus1=bool(opts.get("cus1")), pixel_only=bool(opts.get("pixel_only")))


def photo_losses(c, dtype, leaves=False):
    t = c["target"].to(dtype)
    cs = [x.to(dtype).clone().requires_grad_(leaves) for x in c["cands"]]
    return cs, torch.cat([O.compute_reprojection_loss(x, t, no_ssim=bool(c["flags"] & F_NO_SSIM)) for x in cs], 1)


def ref_photo_decisions(c, dtype=F64):
    """-> r (B,n,H,W), rp, argmin, weight of the reference's own decisions, and the automask's margin rp - ident'"""
    _, r = photo_losses(c, dtype)
    if c["flags"] & F_AVG:
        rp, am = r.mean(1, True), torch.full_like(r[:, :1], 255).long()
    else:
        rp, am = torch.min(r, 1, keepdim=True)
    w, margin = torch.ones_like(rp), None
    if c["flags"] & F_AUTOMASK:
        idn = c["ident"].to(dtype) + (c["noise"].to(dtype) * 0.00001 if c["noise"] is not None else 0)
        w, margin = (rp <= idn).to(dtype), rp - idn
    if c["ext"] is not None:
        w = w * c["ext"].to(dtype)
    return r.detach(), rp.detach(), am, w, margin


def ref_photo_forced(c, dtype, am, wt, sums1):
    """sum(rp w) and d/d cand_c x scale / (sums[1] + 1e-7) with the device's ``am`` (B,1,H,W long) and ``wt`` forced"""
    cs, r = photo_losses(c, dtype, leaves=True)
    rp = r.mean(1, True) if c["flags"] & F_AVG else torch.gather(r, 1, am.clamp(max=r.shape[1] - 1))
    s = (rp * wt.to(dtype)).sum()
    s.backward()
    k = float(c["scale"]) / (sums1 + 1e-7)
    grads = {"g_cand%d" % i: ((x.grad if x.grad is not None else torch.zeros_like(x)) * k if c["need"][i] else None)
             for i, x in enumerate(cs)}
    return dict(sum_rw=s.detach().reshape(1)), grads


# ================================================================ 6. smooth_loss
# name: (B, C, H, W).  Marching route (C = 3, option photo_impl = 1): 62-column strips x 12-row segments, the finish kernel
# takes samples 16 and tasks 64 at a time.  Pixel route: any other C, and C = 3 under photo_impl = 0.
SMOOTH_CASES = {
    "march_b1_2x2": (1, 3, 2, 2), "march_b1_11x61": (1, 3, 11, 61), "march_b16_12x62": (16, 3, 12, 62),
    "march_b17_13x63": (17, 3, 13, 63), "march_b1_25x124": (1, 3, 25, 124), "march_b1_25x125": (1, 3, 25, 125),
    "march_b1_265x125_69_tasks_per_sample": (1, 3, 265, 125),
    "pixel_c1_2x2": (1, 1, 2, 2), "pixel_c2_13x63": (3, 2, 13, 63), "pixel_c4_25x125": (1, 4, 25, 125),
    "pixel_c1_b100_72x104_chunk_cap_bites": (100, 1, 72, 104),
}
SMOOTH_PIXEL_C3 = ("march_b1_2x2", "march_b17_13x63", "march_b1_25x125")   # run again under photo_impl = 0
SMOOTH_REFUSED, SMOOTH_LAST_ACCEPTED = (586, 1, 2, 2), (585, 1, 2, 2)
CONSTANT_SAMPLE = 1   # of a batch: not the last one, which at B = 17 is the sample the finish kernel takes in its second round


def smooth_tasks(H, W):
    return (W + 61) // 62, (H + 11) // 12


def smooth_chunks(B, H, W):
    """pixel route -> (chunks wanted, the cap): the scratch holds 4096 doubles, B chunks (1 + 4) + 2 B of them are used"""
    return (H * W + 1023) // 1024, (4096 - 2 * B) // 5 // B


def smooth_case(name):
    B, C, H, W = SMOOTH_CASES[name]
    g = gen(name)
    # disparities are a sigmoid's range, POSITIVE: the marching sweep factors the positive per-sample mean out of the sign
    disp = torch.sigmoid(torch.randn(B, 1, H, W, generator=g) - 1.0)
    disp[0, 0, 0, 1] = disp[0, 0, 0, 0]                         # a tie along a row
    disp[0, 0, 1, W - 1] = disp[0, 0, 0, W - 1]                 # and along a column
    if B > 1:
        disp[CONSTANT_SAMPLE] = 0.25                            # a constant sample: every difference a tie
    assert float(disp.min()) > 0
    return dict(disp=disp.contiguous(), img=torch.rand(B, C, H, W, generator=g))


def ref_smooth(c, dtype, normalise):
    d = c["disp"].to(dtype).clone().requires_grad_(True)
    loss = (O.normalized_smooth_loss if normalise else O.get_smooth_loss)(d, c["img"].to(dtype))
    loss.backward()
    return dict(loss=loss.detach().reshape(1)), dict(g_disp=d.grad)


# ================================================================ 7. distillation epilogue
# name: (B, H, W, flags, options)
DISTIL_CASES = {
    "n4_two_way": (1, 2, 2, 0, {}),
    "n4_three_way_dual": (1, 2, 2, F_DUAL_DISTIL, dict(ens=True, ext=True)),
    "n258_three_way": (1, 2, 129, 0, dict(ens=True, ext=True)),          # check_shape refuses 1 x 257; 258 straddles 256 too
    "n258_two_way_dual_no_target": (1, 2, 129, F_DUAL_DISTIL, dict(ext=True, want_ct=False)),
    "n258_learned": (1, 2, 129, 0, dict(ens=True, ext=True, learned=True)),
    "n258_learned_no_mask_no_grad": (1, 2, 129, 0, dict(ens=True, learned=True, need_grad=False)),
    "n589824_three_way_dual_past_2048_blocks": (3, 384, 512, F_DUAL_DISTIL, dict(ens=True, ext=True)),
}


def distil_case(name):
    B, H, W, flags, opts = DISTIL_CASES[name]
    g = gen(name)
    new = lambda lo, hi: (lo + (hi - lo) * torch.rand(B, 1, H, W, generator=g))
    c = dict(multi_depth=new(0.5, 20), mono_depth=new(0.5, 20), multi_reproj=new(0, 0.3), mono_reproj=new(0, 0.3),
             ens_reproj=new(0, 0.3) if opts.get("ens") else None, ens_depth=new(0.5, 20) if opts.get("learned") else None,
             ext=(torch.rand(B, 1, H, W, generator=g) < 0.7).float() if opts.get("ext") else None, flags=flags,
             need_grad=opts.get("need_grad", True), want_ct=opts.get("want_ct", True))
    f = lambda k: c[k].view(-1)
    if c["ens_reproj"] is not None:
        f("ens_reproj")[0] = f("mono_reproj")[0]                      # mono == ens: mono wins
        f("multi_reproj")[0] = 1.0
        f("multi_reproj")[1] = f("ens_reproj")[1] = 0.0               # ens == multi (< mono): the ensemble stays the winner
        f("mono_reproj")[1] = 0.5
    else:
        f("multi_reproj")[1] = f("mono_reproj")[1]                    # mono == multi: mono wins
    f("multi_depth")[2] = f("mono_depth")[2]                          # sign 0
    if c["ext"] is not None:  # the crafted pixels count: weight 1 under the winner's ties, 1 - weight = 1 under the depth tie
        f("ext")[:3] = torch.tensor([1.0, 1.0, 0.0])
    return c


def ref_distil(c, dtype):
    """mal_distil_epilogue's contract (include/mal_hip.h, distil_kernel) in tensor operations: w = ext_mask (1 without);
    sums[2] = sum |multi - mono| (1 - w); the winner of (mono, ens, multi) reprojection, first minimum first, names the
    distillation target among (mono, (mono + multi) / 2 or ens_depth, multi); sums[3] = sum |target - multi| w; the target is
    detached except the ensemble's own dependence on multi and, with --dual_distil, the mono target."""
    dual, learned = bool(c["flags"] & F_DUAL_DISTIL), c["ens_depth"] is not None
    lv = {k: c[k].to(dtype).clone().requires_grad_(True) for k in ("multi_depth", "mono_depth")}
    ens_d = c["ens_depth"].to(dtype).clone().requires_grad_(True) if learned else None
    dm, dmono = lv["multi_depth"], lv["mono_depth"]
    w = c["ext"].to(dtype) if c["ext"] is not None else torch.ones_like(dm)
    cons = ((dm - dmono.detach()).abs() * (1 - w)).sum()
    cand = [c["mono_reproj"], c["ens_reproj"] if c["ens_reproj"] is not None else torch.full_like(c["mono_reproj"], math.inf),
            c["multi_reproj"]]
    idx = torch.argmin(torch.stack(cand, 0).to(dtype), 0)             # first minimum wins, as the kernel's strict <
    mono_t = dmono if dual else dmono.detach()
    ens = ens_d if learned else (dmono.detach() + dm) / 2
    target = torch.where(idx == 0, mono_t, torch.where(idx == 2, dm.detach(), ens))
    dist = ((target - dm).abs() * w).sum()
    g_cons = torch.autograd.grad(cons, dm, retain_graph=True)[0]
    wanted = [dm] + ([dmono] if dual else []) + ([ens_d] if learned else [])
    got = torch.autograd.grad(dist, wanted, allow_unused=True)
    got = [torch.zeros_like(dm) if x is None else x for x in got]
    out = dict(sums=torch.stack([cons, dist]).detach(), g_cons=g_cons, g_dist=got[0],
               g_4th=got[1] if (dual or learned) else None,
               cons_target=(1 / (dmono * (1 - w) + dm * w)).detach(), idx=idx)
    return out


# ================================================================ 8. axpy_maps, finish_scalars, sum_f64
# name: (n, terms, accumulate, out given);  terms: (scale?, denom?, eps) each
AXPY_CASES = {
    "n1_one_term": (1, [(False, False, 0.0)], False, False),
    "n257_two_terms_accumulate": (257, [(True, True, 1e-7), (False, True, 0.0)], True, True),
    "n257_six_terms": (257, [(True, True, 1e-7), (True, False, 0.0), (False, True, 0.5), (False, False, 0.0),
                              (True, True, 0.0), (True, False, 0.0)], False, True),
    "n600000_six_terms_accumulate_past_2048_blocks": (600000, [(True, True, 1e-7), (True, False, 0.0), (False, True, 0.5),
                                                               (False, False, 0.0), (True, True, 0.0), (True, False, 0.0)], True, True),
}
SUM_N = (1, 63, 65, 262144, 262145, 1200003)


def axpy_case(name):
    n, terms, acc, has_out = AXPY_CASES[name]
    g = gen(name)
    k = len(terms)
    return dict(maps=[torch.randn(n, generator=g) for _ in range(k)],
                scales=[(0.5 + torch.rand(1, generator=g)) if t[0] else None for t in terms],
                denoms=[(10 + 1000 * torch.rand(1, generator=g, dtype=F64)) if t[1] else None for t in terms],
                mults=[float(np.float32(x)) for x in (torch.randn(k, generator=g)).tolist()], eps=[t[2] for t in terms],
                out=torch.randn(n, generator=g) if has_out else None, accumulate=acc and has_out)


def ref_axpy(c):
    """-> (the value with float32-rounded coefficients in float64, the per-element bound)"""
    n = c["maps"][0].numel()
    acc = c["out"].double().clone() if c["accumulate"] else torch.zeros(n, dtype=F64)
    mag = acc.abs().clone()
    for m, s, d, mult, eps in zip(c["maps"], c["scales"], c["denoms"], c["mults"], c["eps"]):
        coef = float(np.float32(mult)) * (float(s) if s is not None else 1.0)
        if d is not None:
            coef = coef / (float(d) + float(np.float32(eps)))
        coef = float(np.float32(coef))
        acc, mag = acc + coef * m.double(), mag + (coef * m.double()).abs()
    return acc, (len(c["maps"]) + 2) * EPS24 * mag


def sum_case(n):
    g = torch.Generator().manual_seed(n % 9973)
    x = torch.randn(n, generator=g) * torch.pow(10.0, 6 * torch.rand(n, generator=g) - 3)   # mixed sign, 1e-3 .. 1e3
    return x.contiguous()


def sum_bound(x):
    return x.numel() * 2.0 ** -53 * float(x.double().abs().sum())


# ================================================================ 9. pose
# name: (B, F, inverts, need_aa, need_tr)
POSE_CASES = {
    "b1_f1": (1, 1, (False,), (True,), (True,)),
    "b1_f2_mixed_invert": (1, 2, (True, False), (True, False), (False, True)),
    "b65_f1_invert": (65, 1, (True,), (True,), (True,)),
    "b65_f2_mixed_invert": (65, 2, (False, True), (False, True), (True, True)),
}


def pose_case(name):
    B, Fr, inv, need_aa, need_tr = POSE_CASES[name]
    g = gen(name)
    aa = [0.3 * torch.randn(B, 1, 3, generator=g) for _ in range(Fr)]
    tr = [0.5 * torch.randn(B, 1, 3, generator=g) for _ in range(Fr)]
    aa[0][0] = 0.0                                                   # exactly zero: d|v|/dv = 0 there, as torch.norm
    if B > 2:
        aa[0][1] = torch.tensor([[6e-7, -6e-7, 5.2915e-7]])           # norm 1e-6: the reference divides by norm + 1e-7
        aa[0][2] = 0.01 * aa[0][2]
    return dict(aa=aa, tr=tr, inv=inv, need_aa=need_aa, need_tr=need_tr, g_T=[torch.randn(B, 4, 4, generator=g) for _ in range(Fr)])


def ref_pose(c, dtype):
    out, grads = {}, {}
    for f, (a, t) in enumerate(zip(c["aa"], c["tr"])):
        a, t = a.to(dtype).clone().requires_grad_(True), t.to(dtype).clone().requires_grad_(True)
        T = O.transformation_from_parameters(a, t, c["inv"][f])
        (T * c["g_T"][f].to(dtype)).sum().backward()
        out["T%d" % f] = T.detach()
        grads["g_aa%d" % f] = a.grad if c["need_aa"][f] else None
        grads["g_tr%d" % f] = t.grad if c["need_tr"][f] else None
    return out, grads


# ================================================================ admissibility, shared
def admissible(ref64, ref32, forward=False, floor=1e-4, what=""):
    """the float32 torch reference alone inside the gate at ``floor`` (``check`` with no float32 allowance to add)"""
    return check(ref32, ref64, None, forward=forward, floor=floor, what=what)
