"""TEST INFRASTRUCTURE: DynamicDepth's ``forward_warp`` (dynamicdepth/rigid_warp.py:534-597) restated in torch for any
float dtype, the case table of the forward-warp tests, and their checkers.

The restatement is split where the kernels are: ``splat`` (the z-buffer and, per sub-point, x, y, the cell and 1/Z) and
``resolve(zbuf, ...)`` (depth_w, the inverse warp, the three outputs).  In fp32 it reproduces the reference bit for bit
(tests/golden/fwarp_*.npz, scripts/gen_golden_fwarp.py); in fp64 it is the decision reference of every gate, because the
reference itself cannot run in fp64 (its cached pixel grid keeps the first dtype and ``sparse.FloatTensor`` is fp32 only).

Where the restatement is NOT upstream's text: the range test.  Upstream truncates with ``.long()`` and then sends indices
``< 0`` or ``> hh-1`` to a dump row.  For finite coordinates that is ``x > -1 && x < W && y > -1 && y < H`` on the floats
(coordinates in (-1, 0) truncate to cell 0), which is what is written here and in the kernel; for NaN and +-inf ``.long()``
is undefined and the float test is the definition: they land nowhere.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the project's cap on differing decisions: 3e-4 N + 8
def cap(n):
    return 3e-4 * n + 8


X_EDGE_TOL = 1e-4   # a sub-point is a near-tie when x or y (fp64) is within this of a truncation edge
COORD_TOL = 1e-5    # iw_val: |coord| (fp64) within this of 1


# ---- upstream's small matrices, restated ------------------------------------------------------------------------------------
def euler_to_mat(angle):
    """(B,3) angles about x, y, z -> (B,3,3) = Rx Ry Rz"""
    x, y, z = angle[:, 0], angle[:, 1], angle[:, 2]
    zero, one = z * 0, z * 0 + 1
    rz = torch.stack([z.cos(), -z.sin(), zero, z.sin(), z.cos(), zero, zero, zero, one], 1).reshape(-1, 3, 3)
    ry = torch.stack([y.cos(), zero, y.sin(), zero, one, zero, -y.sin(), zero, y.cos()], 1).reshape(-1, 3, 3)
    rx = torch.stack([one, zero, zero, zero, x.cos(), -x.sin(), zero, x.sin(), x.cos()], 1).reshape(-1, 3, 3)
    return rx @ ry @ rz


def mat_to_euler(R):
    sy = torch.sqrt(R[:, 0, 0] * R[:, 0, 0] + R[:, 1, 0] * R[:, 1, 0])
    s = (sy < 1e-6).to(R.dtype)
    x = torch.atan2(R[:, 2, 1], R[:, 2, 2])
    y = torch.atan2(-R[:, 2, 0], sy)
    z = torch.atan2(R[:, 1, 0], R[:, 0, 0])
    xs = torch.atan2(-R[:, 1, 2], R[:, 1, 1])
    zs = R[:, 1, 0] * 0
    return torch.stack([x * (1 - s) + xs * s, y * (1 - s) + y * s, z * (1 - s) + zs * s], -1)


def pixel_grid(h, w, dtype):
    i = torch.arange(0, h).view(1, h, 1).expand(1, h, w).to(dtype)
    j = torch.arange(0, w).view(1, 1, w).expand(1, h, w).to(dtype)
    return torch.stack((j, i, torch.ones(1, h, w, dtype=dtype)), 1)  # (1,3,h,w): x, y, 1


def back_project(depth, K_inv):
    b, h, w = depth.shape
    pix = pixel_grid(h, w, depth.dtype).expand(b, 3, h, w).reshape(b, 3, -1)
    return (K_inv @ pix).reshape(b, 3, h, w) * depth.unsqueeze(1)


# ---- stage 1 --------------------------------------------------------------------------------------------------------------
def splat(depth, pose, K, up, dtype=torch.float32):
    """depth (B,1,H,W), pose (B,3,4), K (B,3,3) -> dict: zbuf (B,H,W) the largest 1/Z per cell (0 = empty); per sub-point
    (B, up H * up W) x, y, inv = 1/Z, cell = ty * W + tx or -1"""
    depth, pose, K = depth.to(dtype), pose.to(dtype), K.to(dtype)
    B, _, H, W = depth.shape
    depth_u = F.interpolate(depth, scale_factor=up).squeeze(1)
    K_u = torch.cat((K[:, 0:2] * up, K[:, 2:]), 1)
    cam = back_project(depth_u, K_u.inverse()).reshape(B, 3, -1)
    moved = pose[:, :, :3] @ cam + pose[:, :, -1:]
    X, Y, Z = moved[:, 0], moved[:, 1], moved[:, 2].clamp(min=1e-3)
    pn = torch.stack([X / Z, Y / Z, Z / Z], 1)
    pix = (K @ pn).permute(0, 2, 1)[:, :, :2]
    x, y = pix[..., 0], pix[..., 1]
    inv = 1 / Z
    inside = (x > -1) & (x < W) & (y > -1) & (y < H)
    tx = torch.where(inside, x, torch.zeros_like(x)).long()
    ty = torch.where(inside, y, torch.zeros_like(y)).long()
    cell = torch.where(inside, ty * W + tx, torch.full_like(tx, -1))
    idx = torch.where(inside, cell, torch.full_like(cell, H * W))
    zbuf = torch.zeros(B, H * W + 1, dtype=dtype).scatter_reduce(1, idx, inv, "amax", include_self=True)[:, :-1]
    return {"zbuf": zbuf.reshape(B, H, W), "x": x, "y": y, "inv": inv, "cell": cell}


# ---- stage 2 --------------------------------------------------------------------------------------------------------------
def inverse_pose_vec(pose):
    """(B,3,4) -> upstream's 6-vector of the inverse: translation, then the Euler angles of the inverse rotation"""
    B = pose.shape[0]
    last = torch.tensor([0, 0, 0, 1], dtype=pose.dtype).view(1, 1, 4).repeat(B, 1, 1)
    inv = torch.inverse(torch.cat([pose, last], 1))
    return torch.cat([inv[:, :3, 3], mat_to_euler(inv[:, :3, :3])], 1)


def inverse_warp(img, depth, pose6, K, dtype=torch.float32):
    """rigid_warp.py:337-373: img (B,C,H,W), depth (B,H,W), pose6 (B,6) -> sampled image, valid_points (bool), coords"""
    img, depth, pose6, K = img.to(dtype), depth.to(dtype), pose6.to(dtype), K.to(dtype)
    B, _, H, W = img.shape
    cam = back_project(depth, K.inverse()).reshape(B, 3, -1)
    proj = K @ torch.cat([euler_to_mat(pose6[:, 3:]), pose6[:, :3].unsqueeze(-1)], 2)
    p = proj[:, :, :3] @ cam + proj[:, :, -1:]
    X, Y, Z = p[:, 0], p[:, 1], p[:, 2].clamp(min=1e-3)
    coords = torch.stack([2 * (X / Z) / (W - 1) - 1, 2 * (Y / Z) / (H - 1) - 1], 2).reshape(B, H, W, 2)
    out = F.grid_sample(img, coords, padding_mode="zeros", align_corners=True)
    return out, coords.abs().max(-1)[0] <= 1, coords


def resolve(zbuf, img, pose, K, dtype=torch.float32):
    """zbuf (B,H,W) as ``splat`` (or a kernel) left it -> dict img_w, depth_w (B,1,H,W), valid (B,1,H,W), all masked as
    upstream returns them, plus fw_val, iw_val (bool) and coords (B,H,W,2)"""
    zbuf = zbuf.to(dtype)
    fw = zbuf != 0
    depth_w = torch.where(fw, 1 / torch.where(fw, zbuf, torch.ones_like(zbuf)), torch.zeros_like(zbuf))
    img_s, iw, coords = inverse_warp(img, depth_w, inverse_pose_vec(pose.to(dtype)), K, dtype)
    valid = (fw.to(dtype) * iw.to(dtype)).unsqueeze(1)
    return {"img_w": img_s * valid, "depth_w": depth_w.unsqueeze(1) * valid, "valid": valid, "fw_val": fw, "iw_val": iw,
            "coords": coords, "depth_raw": depth_w}


def forward_warp(img, depth, pose, K, up, dtype=torch.float32):
    s = splat(depth, pose, K, up, dtype)
    r = resolve(s["zbuf"], img, pose, K, dtype)
    r.update(splat=s)
    return r


def compose(dst, img_w, mask, no_reproj=False):
    """trainer.py:506-510 with upstream's index assignments; mask (B,1,H,W) or None"""
    dst = dst.clone()
    if mask is not None:
        dst[mask.repeat(1, dst.shape[1], 1, 1) == 1] = 0
    if no_reproj:
        dst[img_w > 0] = 0
    else:
        dst[img_w > 0] = img_w[img_w > 0]
    return dst


# ---- the case table -------------------------------------------------------------------------------------------------------
# name -> (B, H, W, C, upscale, content, seed, per_sample_K)
REFERENCE_SHAPES = [(2, 24, 72), (3, 37, 50), (2, 5, 7)]
CASES = {}
for _b, _h, _w in REFERENCE_SHAPES:
    for _s in range(4):
        CASES["ref_b%d_%dx%d_s%d" % (_b, _h, _w, _s)] = (_b, _h, _w, 3, 3, "generic", _s, False)
for _u in (1, 2, 3, 4):
    CASES["lattice_generic_u%d" % _u] = (2, 24, 72, 3, _u, "identity", 0, False)
    CASES["lattice_pow2_u%d" % _u] = (2, 8, 32, 3, _u, "identity_pow2", 0, False)
GOLDEN_CASES = list(CASES)  # the 20 cases the reference itself was run on
CASES.update({
    "tiny_2x2": (1, 2, 2, 3, 3, "generic", 0, False),
    "w63": (1, 3, 63, 3, 3, "generic", 1, False),
    "w64": (1, 3, 64, 3, 3, "generic", 2, False),
    "w65": (1, 3, 65, 3, 3, "generic", 3, False),
    "h3_up1": (2, 3, 9, 1, 1, "generic", 4, False),      # below the tile height of 4
    "h4_up2": (2, 4, 9, 4, 2, "generic", 5, True),       # exactly one tile row
    "h5_up4": (2, 5, 70, 3, 4, "generic", 6, True),      # a ragged second tile row and a second tile column
    "c1_per_k": (2, 24, 72, 1, 3, "generic", 7, True),
    "c4_per_k": (3, 37, 50, 4, 2, "generic", 8, True),
    "large_motion": (2, 24, 72, 3, 3, "large_motion", 0, False),
    "parallax_split": (2, 24, 72, 3, 3, "parallax_split", 0, False),
    "converge": (2, 24, 72, 3, 3, "converge", 0, False),
    "diverge": (2, 24, 72, 3, 3, "diverge", 0, False),
    "behind_camera": (2, 24, 72, 3, 3, "behind_camera", 0, False),
    "all_outside": (2, 5, 7, 3, 3, "all_outside", 0, False),
})
GPU_CASES = [k for k in CASES if not k.startswith("ref_b2_24x72_s") or k.endswith("s0")]


def _euler_np(a):
    cx, sx, cy, sy, cz, sz = math.cos(a[0]), math.sin(a[0]), math.cos(a[1]), math.sin(a[1]), math.cos(a[2]), math.sin(a[2])
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rx @ ry @ rz


def make_case(name):
    """-> dict of fp32 CPU tensors img (B,C,H,W), depth (B,1,H,W), pose (B,3,4), K (B,3,3), and up.
    generic: pose = euler2mat(0.01 N), t = 0.05 N, depth = 1 / (0.01 + 9.99 U), K = [[0.58 W, 0, 0.5 W], [0, 1.92 H, 0.5 H],
    [0, 0, 1]]: the content the CPU gates were measured on."""
    B, H, W, C, up, kind, seed, per_k = CASES[name]
    rng = np.random.default_rng(9100 + 17 * seed + 1000 * H + W)
    K = np.tile(np.array([[0.58 * W, 0, 0.5 * W], [0, 1.92 * H, 0.5 * H], [0, 0, 1]]), (B, 1, 1))
    if kind == "identity_pow2":
        K = np.tile(np.array([[32.0, 0, 16], [0, 64, 8], [0, 0, 1]]), (B, 1, 1))
    if per_k:
        K[:, 0, 0] *= 1 + 0.2 * rng.random(B)
        K[:, 1, 1] *= 1 - 0.2 * rng.random(B)
        K[:, :2, 2] += rng.standard_normal((B, 2))
    ang, t = 0.01 * rng.standard_normal((B, 3)), 0.05 * rng.standard_normal((B, 3))
    depth = 1.0 / (0.01 + 9.99 * rng.random((B, 1, H, W)))
    img = rng.random((B, C, H, W))
    if kind in ("identity", "identity_pow2"):
        ang, t = ang * 0, t * 0
    if kind == "identity_pow2":       # depths that are powers of two as well: (a d) / d is then exact in any precision
        depth = 2.0 ** rng.integers(-2, 4, (B, 1, H, W))
    elif kind == "large_motion":      # sub-points leave through every border: a roll and a yaw of opposite sign per sample
        ang, t = 5 * ang, 5 * t
        ang[:, 2] = np.array([0.35, -0.35, 0.2])[:B]
        ang[:, 1] = np.array([0.15, -0.15, 0.1])[:B]
    elif kind == "parallax_split":    # the near half moves by about W/3 (f t_x / Z = 0.58 W t_x / 0.1), the rest by < 1 px
        near = rng.random((B, 1, H, W)) < 0.5
        depth = np.where(near, 0.1, 40.0 + 10 * rng.random((B, 1, H, W)))
        t = np.zeros((B, 3))
        t[:, 0] = 1.013 * 0.1 / (3 * 0.58)  # (not a whole number of pixels: the identity pose's lattice is no decision case)
    elif kind == "converge":          # the camera backs away: the scene shrinks towards the centre, many sub-points per cell
        depth = 1.0 + rng.random((B, 1, H, W))
        t[:, 2] = 2.0
    elif kind == "diverge":           # the camera advances: the scene spreads, mostly holes
        depth = 2.0 + rng.random((B, 1, H, W))
        t[:, 2] = -1.9
    elif kind == "behind_camera":     # a third of the scene ends at Z = 5e-4 < 1e-3: the clamp makes 1/Z = 1000 and doubles
        depth = np.where(rng.random((B, 1, H, W)) < 0.33, 0.002, 2.0 + rng.random((B, 1, H, W)))  # its offset from the centre
        t = np.zeros((B, 3))
        t[:, 2] = -0.0015
    elif kind == "all_outside":
        ang = ang * 0
        t = np.zeros((B, 3))
        t[:, 0] = 1e4
    pose = np.concatenate([np.stack([_euler_np(a) for a in ang]), t[:, :, None]], 2)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return {"img": T(img), "depth": T(depth), "pose": T(pose), "K": T(K), "up": up}


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, "fwarp_%s.npz" % name), allow_pickle=False)
    return {k: z[k] for k in z.files}


# ---- checkers -------------------------------------------------------------------------------------------------------------
def near_edge(v, size):
    """fp64 coordinates -> True where within X_EDGE_TOL of a truncation edge: -1, 1, 2, ..., size (0 is not an edge:
    (-1, 1) truncates to one cell)"""
    v = np.asarray(v, np.float64)
    r = np.round(v)
    return (np.abs(v - r) <= X_EDGE_TOL) & (r != 0) & (r >= -1) & (r <= size)


def check_cells(s_test, s64, H, W):
    """sub-point cells of a test splat against the fp64 restatement's: at most cap(N) differ, each a near-tie.  -> count"""
    a, b = s_test["cell"].numpy(), s64["cell"].numpy()
    diff = a != b
    n = int(diff.sum())
    assert n <= cap(a.size), "%d of %d sub-point cells differ (cap %.0f)" % (n, a.size, cap(a.size))
    tie = near_edge(s64["x"].numpy(), W) | near_edge(s64["y"].numpy(), H)
    assert not (diff & ~tie).any(), "%d differing sub-points are not near a truncation edge" % int((diff & ~tie).sum())
    return n


def near_tie_cells(s64, H, W):
    """(B,H,W) bool: cells that hold, or touch (3x3), the fp64 cell of a near-tie sub-point, plus the border cells a near-tie
    at the range limits -1, W, H could have entered"""
    x, y, cell = s64["x"].numpy(), s64["y"].numpy(), s64["cell"].numpy()
    tie = near_edge(x, W) | near_edge(y, H)
    B = x.shape[0]
    m = np.zeros((B, H + 2, W + 2), bool)
    bi, si = np.nonzero(tie)
    cx = np.clip(np.round(x[bi, si]), -1, W).astype(np.int64)  # the edge itself: both sides are within one cell of it
    cy = np.clip(np.round(y[bi, si]), -1, H).astype(np.int64)
    ok = np.isfinite(x[bi, si]) & np.isfinite(y[bi, si])
    bi, cx, cy = bi[ok], cx[ok], cy[ok]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            m[bi, np.clip(cy + 1 + dy, 0, H + 1), np.clip(cx + 1 + dx, 0, W + 1)] = True
    return m[:, 1:-1, 1:-1]


def check_zbuf(z_test, s32, s64, H, W):
    """Splat gate: a cell differs when off by more than max(1e-6, 1.25 x the fp32 restatement's own distance) relative; at
    most cap(N) cells may, each explained by a near-tie sub-point in it or next to it.  -> (differing cells, gate)"""
    z64 = s64["zbuf"].numpy()
    z32 = s32["zbuf"].numpy().astype(np.float64)
    zt = np.asarray(z_test, np.float64)
    both = (z64 != 0) & (z32 != 0)
    # the fp32 restatement's own distance is taken where it made the fp64 decisions; its near-tie cells are judged like the kernel's
    ties = near_tie_cells(s64, H, W)
    calm = both & ~ties
    own = float(np.max(np.abs(z32 - z64)[calm] / z64[calm])) if calm.any() else 0.0
    gate = max(1e-6, 1.25 * own)
    off = np.abs(zt - z64) > gate * np.maximum(np.abs(z64), 1e-30)
    off |= (zt != 0) != (z64 != 0)
    n = int(off.sum())
    N = s64["cell"].numel()
    assert n <= cap(N), "%d z-buffer cells differ (cap %.0f)" % (n, cap(N))
    assert not (off & ~ties).any(), "%d differing z-buffer cells have no near-tie sub-point in or next to them; worst %.3g (gate %.3g)" % (
        int((off & ~ties).sum()), float(np.max((np.abs(zt - z64) / np.maximum(np.abs(z64), 1e-30))[off & ~ties])), gate)
    return n, gate


def check_resolve(out, r32, r64, img_scale, n_sub):
    """Resolve gate, all three on ONE z-buffer: ``out`` = dict img_w, depth_w, valid (numpy, upstream's shapes) of the code
    under test; r32 / r64 the restatement on that z-buffer.  valid may differ at near-ties (|coord| within COORD_TOL of 1)
    under the cap; depth_w within max(1e-5, 1.25 x fp32 distance) relative, img_w within max(1e-4, 1.25 x fp32 distance) of
    the image scale, where valid agrees."""
    v64, v32 = r64["valid"].numpy()[:, 0] != 0, r32["valid"].numpy()[:, 0] != 0
    vt = np.asarray(out["valid"])[:, 0] != 0
    co = np.abs(r64["coords"].numpy()).max(-1)
    tie = np.abs(co - 1) <= COORD_TOL
    dv = vt != v64
    assert dv.sum() <= cap(n_sub), "%d valid flags differ (cap %.0f)" % (dv.sum(), cap(n_sub))
    assert not (dv & ~tie).any(), "%d differing valid flags are not near |coord| = 1" % int((dv & ~tie).sum())
    same, own = ~dv, v32 == v64  # each side is measured wherever IT took the fp64 decision
    d64, d32 = r64["depth_w"].numpy()[:, 0], r32["depth_w"].numpy()[:, 0].astype(np.float64)
    rel = lambda a, m: float((np.abs(a - d64)[m] / np.maximum(np.abs(d64[m]), 1e-30)).max()) if m.any() else 0.0
    own_d, got_d = rel(d32, own), rel(np.asarray(out["depth_w"], np.float64)[:, 0], same)
    gate_d = max(1e-5, 1.25 * own_d)
    assert got_d <= gate_d, "depth_w off by %.3g relative (gate %.3g, fp32 restatement %.3g)" % (got_d, gate_d, own_d)
    i64, i32 = r64["img_w"].numpy(), r32["img_w"].numpy().astype(np.float64)
    sm, om = np.broadcast_to(same[:, None], i64.shape), np.broadcast_to(own[:, None], i64.shape)
    own_i = float(np.abs(i32 - i64)[om].max()) / img_scale if om.any() else 0.0
    got_i = float(np.abs(np.asarray(out["img_w"], np.float64) - i64)[sm].max()) / img_scale if sm.any() else 0.0
    gate_i = max(1e-4, 1.25 * own_i)
    assert got_i <= gate_i, "img_w off by %.3g of the image scale (gate %.3g, fp32 restatement %.3g)" % (got_i, gate_i, own_i)
    return {"valid_diff": int(dv.sum()), "depth_rel": got_d, "depth_gate": gate_d, "img": got_i, "img_gate": gate_i}
