"""DynamicDepth's occlusion-aware cost volume (dynamicdepth/networks/resnet_encoder.py:148-249 ``match_features``) restated
in torch, generic in D, C and dtype, and what its tests share: the case builder, the fixture table, the cell-level ambiguity
set and the GPU sweep's case table.  TEST INFRASTRUCTURE ONLY.

Written from the semantics of DESIGN.md 17, not from the reference's text; scripts/gen_golden_dyn_costvol.py holds it to the
reference's own fp32 ``match_features`` BIT FOR BIT on the ten fixtures tests/golden/dyn_costvol_*.npz.  fp64 is the exact side
of the GPU gates.

  1. occ = nearest resize to 48x128 of [sum of the lookup image's channels < 0.15], per flattened (B*F) image.
  2. per (b, f), only when aug_mask[b] == 0 and (set_1 or pool): m(d,y,x) = bilinear sample (zeros, align_corners) of
     occ[b] > 0 -- FLAT index b, upstream's indexing -- at the cell's sampling position, > pool_th (strict);
     set_1: warped[m] = 1 on every channel; else pool: warped[m] = max_pool3d over (bin, y, x) of warped with m zeroed.
  3. border masks and the channel mean of |warped - current| as ManyDepth.
  4. cv_min: volume starts at 1, per frame zeros read as 1 and the minimum is kept, a final 1 reads as 0; else the mean
     over the frames that hit.
  5. missing = (volume == 0), optionally filled with the pixel's maximum.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OCC_H, OCC_W = 48, 128
TH_TOL = 2e-4  # |m_value - pool_th| within this (fp64) may fall on either side in fp32

# the five option rows of the fixtures: cv_min, set_1, pool, pool_r, pool_th
OPTION_ROWS = {
    "default": dict(cv_min=True, set_1=False, pool=True, pool_r=1, pool_th=0.7),
    "pool_r2": dict(cv_min=True, set_1=False, pool=True, pool_r=2, pool_th=0.4),
    "set_1": dict(cv_min=True, set_1=True, pool=False, pool_r=2, pool_th=0.4),
    "mean_pool": dict(cv_min=False, set_1=False, pool=True, pool_r=1, pool_th=0.7),
    "cv_min": dict(cv_min=True, set_1=False, pool=False, pool_r=2, pool_th=0.4),
}
GOLDEN_SHAPES = {"b2_f2_12x20": (2, 2, 12, 20, 1), "b1_f1_9x70": (1, 1, 9, 70, 2)}  # B, F, h, w, seed; D = 96, C = 64
GOLDEN_CASES = ["%s_%s" % (s, o) for s in GOLDEN_SHAPES for o in OPTION_ROWS]


def nearest_source_index(out_size, in_size):
    """the source index ATen's nearest resize reads for every output index: floor(dst * (float)(in / out)), clamped"""
    scale = np.float32(in_size) / np.float32(out_size)
    idx = np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, in_size - 1)


def occlusion_images(lookup_images):
    """item 1 with the rule above instead of F.interpolate: (N,3,H,W) -> (N,48,128) float {0,1}"""
    dark = (lookup_images.sum(1) < 0.15).float()
    iy = torch.from_numpy(nearest_source_index(OCC_H, dark.shape[1]))
    ix = torch.from_numpy(nearest_source_index(OCC_W, dark.shape[2]))
    return dark[:, iy][:, :, ix]


def linear_bins(D, lo=0.4, hi=9.0):
    return torch.linspace(lo, hi, D)


def make_images(N, H, W, g, n_rect=2, frac=0.33, holes=0.0):
    """bright pixels >= 0.1 per channel, dark ones <= 0.04 per channel (no near-tie at 0.15); ``n_rect`` dark rectangles per
    image of about ``frac`` of either side, plus a share ``holes`` of single dark pixels"""
    img = 0.101 + 0.79 * torch.rand(N, 3, H, W, generator=g)
    dark = torch.zeros(N, H, W, dtype=torch.bool)
    for n in range(N):
        for _ in range(n_rect):
            rh, rw = max(1, int(H * frac)), max(1, int(W * frac))
            y0 = int(torch.randint(0, H - rh + 1, (1,), generator=g))
            x0 = int(torch.randint(0, W - rw + 1, (1,), generator=g))
            dark[n, y0:y0 + rh, x0:x0 + rw] = True
    if holes > 0:
        dark |= torch.rand(N, H, W, generator=g) < holes
    return torch.where(dark.unsqueeze(1), 0.039 * torch.rand(N, 3, H, W, generator=g), img).half().float()  # fp16-representable


def make_case(B, F_, h, w, D, seed, C=64, HW=None, zero_pose=True, aug=None, n_rect=2, frac=0.33, motion=1.0):
    """current / lookup features (fp16-representable), poses, intrinsics at the matching resolution, lookup images
    (``HW``: their size, default 4h x 4w), bins and the augmentation mask.  With B > 1 and F > 1 one pose is all zero; with
    B > 1 the last sample is augmented (``aug`` overrides).  ``motion`` scales the camera motion: with one inner row the
    sampling position has to stay within one pixel of it to pass the border mask."""
    from mal_amd.synthetic import make_batch
    from oracle import mal_oracle as O
    g = torch.Generator().manual_seed(1000 + seed)
    bt = make_batch(B, 4 * h, 4 * w, seed=seed)
    K = bt["K"].clone()
    K[:, 0] /= 4
    K[:, 1] /= 4
    invK = torch.linalg.pinv(K)
    cur = torch.relu(torch.randn(B, C, h, w, generator=g)).half().float()
    look = (cur.unsqueeze(1) + 0.3 * torch.randn(B, F_, C, h, w, generator=g)).relu().half().float()
    poses = torch.stack([O.transformation_from_parameters(bt["axisangle_m1"] * (motion * (i + 1)), bt["translation_m1"] * (motion * (4 * i + 4)), True)
                         for i in range(F_)], 1)
    if zero_pose and B > 1 and F_ > 1:
        poses[0, 1] = 0.0  # a missing lookup frame
    H, W = HW or (4 * h, 4 * w)
    images = make_images(B * F_, H, W, g, n_rect, frac)
    am = torch.zeros(B, 1, 1, 1)
    if aug is not None:
        am[:, 0, 0, 0] = torch.as_tensor(aug, dtype=torch.float32)
    elif B > 1:
        am[B - 1] = 1.0
    return dict(cur=cur, look=look, poses=poses, K=K, invK=invK, images=images, bins=linear_bins(D), aug=am)


def golden_case(name):
    shape, opt = name.split("_", 3)[:3], name.split("_", 3)[3]
    B, F_, h, w, seed = GOLDEN_SHAPES["_".join(shape)]
    c = make_case(B, F_, h, w, 96, seed)
    c.update(OPTION_ROWS[opt])
    return c


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, "dyn_costvol_%s.npz" % name))
    c = {k: torch.from_numpy(z[k].astype(np.float32)) for k in
         ("cur", "look", "poses", "K", "invK", "images", "bins", "aug")}
    for k in ("cv_min", "set_1", "pool"):
        c[k] = bool(z[k])
    c["pool_r"], c["pool_th"] = int(z["pool_r"]), float(z["pool_th"])
    return c, torch.from_numpy(z["cost_volume"]), torch.from_numpy(z["missing"])


def match_features(cur, look, poses, K, invK, images, bins, cv_min=True, aug=None, set_1=False, pool=False, pool_r=2,
                   pool_th=0.4, set_missing_to_max=True, dtype=torch.float32, details=False, occ_index=None):
    """-> (cost_volume (B,D,h,w), missing (B,D,h,w)) in ``dtype``; with ``details`` also the (B,F,D,h,w) sampled occlusion
    values (NaN where no occlusion handling ran).  ``occ_index(b, f)``: which occlusion image a frame reads (default: b)."""
    from oracle import mal_oracle as O
    B, C, h, w = cur.shape
    F_ = look.shape[1]
    D = bins.numel()
    t = lambda x: x.to(dtype)
    cur, look, poses, K, invK = t(cur), t(look), t(poses), t(K), t(invK)
    images = images.reshape(B * F_, 3, *images.shape[-2:])
    occ = F.interpolate((images.sum(1).unsqueeze(1) < 0.15).float(), [OCC_H, OCC_W])  # nearest
    aug = torch.zeros(B) if aug is None else aug.reshape(B, -1)[:, 0]
    warp_depths = t(bins).view(D, 1, 1, 1).expand(D, 1, h, w).contiguous()
    mvals = torch.full((B, F_, D, h, w), float("nan"), dtype=dtype)
    vols, masks = [], []
    for b in range(B):
        cost = torch.ones(D, h, w, dtype=dtype) if cv_min else torch.zeros(D, h, w, dtype=dtype)
        counts = torch.zeros(D, h, w, dtype=dtype)
        world = O.backproject_depth(warp_depths, invK[b:b + 1].expand(D, 4, 4))
        for f in range(F_):
            pose = poses[b:b + 1, f]
            if pose.sum() == 0:
                continue
            pix = O.project_3d(world, K[b:b + 1].expand(D, 4, 4), pose.expand(D, 4, 4), h, w)
            warped = F.grid_sample(look[b:b + 1, f].repeat(D, 1, 1, 1), pix, padding_mode="zeros", mode="bilinear", align_corners=True)
            if aug[b] == 0 and (set_1 or pool):
                o = occ[b if occ_index is None else occ_index(b, f)]
                mv = F.grid_sample(t((o > 0).float()).unsqueeze(0).repeat(D, 1, 1, 1), pix, padding_mode="zeros", mode="bilinear",
                                   align_corners=True)
                mvals[b, f] = mv[:, 0]
                m = (mv > pool_th).expand_as(warped)
                if set_1:
                    warped = torch.where(m, torch.ones_like(warped), warped)
                else:
                    x = torch.where(m, torch.zeros_like(warped), warped)
                    x = F.max_pool3d(x.permute(1, 0, 2, 3), pool_r * 2 + 1, stride=1, padding=pool_r).permute(1, 0, 2, 3)
                    warped = torch.where(m, x, warped)
            xv = (pix[..., 0] / 2 + 0.5) * (w - 1)
            yv = (pix[..., 1] / 2 + 0.5) * (h - 1)
            edge = ((xv >= 2.0) * (xv <= w - 2) * (yv >= 2.0) * (yv <= h - 2)).to(dtype)
            inner = torch.zeros_like(edge)
            inner[:, 2:-2, 2:-2] = 1.0
            diffs = torch.abs(warped - cur[b:b + 1]).mean(1) * (edge * inner)
            if cv_min:
                diffs = torch.where(diffs == 0, torch.ones_like(diffs), diffs)
                cost = torch.minimum(diffs, cost)
            else:
                cost = cost + diffs
                counts = counts + (diffs > 0).to(dtype)
        if cv_min:
            cost = torch.where(cost == 1, torch.zeros_like(cost), cost)
        else:
            cost = cost / (counts + 1e-7)
        missing = (cost == 0).to(dtype)
        if set_missing_to_max:
            cost = cost * (1 - missing) + cost.max(0)[0].unsqueeze(0) * missing
        vols.append(cost)
        masks.append(missing)
    out = torch.stack(vols, 0), torch.stack(masks, 0)
    return out + (mvals,) if details else out


def run_case(c, dtype=torch.float32, set_missing_to_max=True, details=False, **over):
    a = dict(c)
    a.update(over)
    return match_features(a["cur"], a["look"], a["poses"], a["K"], a["invK"], a["images"], a["bins"], a["cv_min"], a["aug"],
                          a["set_1"], a["pool"], a["pool_r"], a["pool_th"], set_missing_to_max, dtype, details)


def ambiguous_cells(c, mvals64):
    """(B,D,h,w) bool: cells whose result may legitimately differ between fp32 and fp64 -- a cell of the (2r+1)^3 window
    (the cell alone under set_1) samples the occlusion image within TH_TOL of pool_th in some frame, or the cell's own sampling
    position lies in the border band of tests/costvol_checks.py"""
    from tests.costvol_checks import ambiguous
    B, _, h, w = c["cur"].shape
    amb = ambiguous(c["poses"], c["K"], c["invK"], c["bins"], B, h, w)
    if c["set_1"] or c["pool"]:
        near = ((mvals64 - c["pool_th"]).abs() <= TH_TOL).any(1).float()  # NaN (no handling) compares False
        r = 0 if c["set_1"] else c["pool_r"]
        if r:
            near = F.max_pool3d(near.unsqueeze(1), 2 * r + 1, stride=1, padding=r)[:, 0]
        amb = amb | (near > 0)
    return amb


# ---- the GPU sweep's cases against the restatement: name -> (make_case arguments, options).  The smallest at which the
# kernels can still go wrong: D around the 6 bins a wavefront owns and the depth window clipped at both ends (1, 2, 3, 5, 7,
# 13), D = 96 and D > 96; 65 / 63 / 64 pixels around a wavefront, one inner row (5 x 13, 5 x 70); lookup images that are not
# 4h x 4w; F = 1..3 under the occ[b] rule; r = 0..2; thresholds that mask everything / nothing; all-black and no-black images.
_DEF = OPTION_ROWS["default"]
_R2 = OPTION_ROWS["pool_r2"]
SWEEP = {
    "D1_5x13": (dict(B=1, F_=1, h=5, w=13, D=1, seed=11, motion=0.2), _R2),
    "D2_7x9": (dict(B=1, F_=2, h=7, w=9, D=2, seed=12), _R2),
    "D3_8x8": (dict(B=2, F_=1, h=8, w=8, D=3, seed=13), _DEF),
    "D5_5x70": (dict(B=1, F_=1, h=5, w=70, D=5, seed=31), _R2),
    "D7_16x28": (dict(B=2, F_=3, h=16, w=28, D=7, seed=15), _DEF),
    "D13_7x9_r0": (dict(B=1, F_=2, h=7, w=9, D=13, seed=16), dict(_DEF, pool_r=0)),
    "D96_16x28": (dict(B=1, F_=2, h=16, w=28, D=96, seed=17, zero_pose=False), _R2),
    "D100_8x8": (dict(B=1, F_=1, h=8, w=8, D=100, seed=18), _DEF),
    "img_37x50": (dict(B=2, F_=2, h=8, w=8, D=7, seed=19, HW=(37, 50)), _DEF),
    "img_200x130": (dict(B=1, F_=3, h=7, w=9, D=5, seed=20, HW=(200, 130)), _R2),
    "F3_occ_b": (dict(B=3, F_=3, h=8, w=8, D=5, seed=21, zero_pose=False, aug=[0, 0, 0]), _DEF),
    "mean_r2": (dict(B=2, F_=2, h=16, w=28, D=13, seed=22), dict(_R2, cv_min=False)),
    "th_below_0": (dict(B=1, F_=2, h=7, w=9, D=5, seed=23), dict(_DEF, pool_th=-0.5)),
    "th_above_1": (dict(B=1, F_=2, h=7, w=9, D=5, seed=24), dict(_DEF, pool_th=1.01)),  # at exactly 1 a fully dark neighbourhood is a tie
    "set_1_th_below_0": (dict(B=1, F_=1, h=7, w=9, D=5, seed=25), dict(OPTION_ROWS["set_1"], pool_th=-0.5)),
    "all_black": (dict(B=1, F_=2, h=7, w=9, D=5, seed=26, n_rect=1, frac=1.0), _R2),
    "no_black": (dict(B=1, F_=2, h=7, w=9, D=5, seed=27, n_rect=0), _R2),
    "set_1_zero_feats": (dict(B=1, F_=1, h=8, w=8, D=3, seed=28, n_rect=1, frac=1.0), OPTION_ROWS["set_1"]),
}


def sweep_case(name):
    args, opt = SWEEP[name]
    c = make_case(**args)
    c.update(opt)
    if name == "set_1_zero_feats":  # a masked pixel whose current features are all 0: the cost is exactly 1 = missing
        c["cur"][:, :, 3, 3] = 0.0
    return c
