"""What the epipolar sweep shares (tests/test_epipolar_cases.py on the CPU, tests/test_gpu_epipolar_sweep.py on the device):
the case table, the case generator, the fp64 / fp32 references and the gate.

The gate is the project's existing one (README "Parity"), nothing looser: a tensor is held within
``max(1e-4, 1.25 x the fp32 oracle's own distance from the fp64 oracle)`` of the fp64 oracle, distances being max |.|
relative to the fp64 tensor's largest magnitude.  Per-pixel gradient maps get the tap-boundary allowance of
``tests/test_gpu_epipolar.py::check_grads`` as it stands (a sample within rounding distance of a tap boundary takes the
neighbouring taps: the value is continuous there, the slope is not): at most ``2e-4 + 4/numel`` of the elements outside,
and L2 relative <= 2e-3.  Forward values get no allowance.  The allowance is a condition on the INPUTS: ``admissible``
holds the fp32 oracle itself to the plain 1e-4 form of the gate, and tests/test_epipolar_cases.py asserts it for every
case of the table."""
import zlib
from types import SimpleNamespace

import numpy as np
import torch

from oracle import epi_oracle as E
from oracle.gen_golden_epi import make_case

DEV = "cuda:0"
DELTA = 0.7
LEAVES = ("depth", "poses", "delta", "f1", "f2")
FORWARD = ("coords", "max_dx", "ds", "corr")
SUM_FLOOR = 2.5e-5

# ---------------------------------------------------------------- the case table: (B, C, h, w, r, L, heads), options
# LDS bands: the lookup's accumulators take sum_l (h>>l)(w>>l) x 8 bytes, the align step's h w x 8
LOOKUP_CASES = {
    # tails and pyramids: d1 mod 3 = 1 (r = 3, 6) and 0 (r = 1), L = 4, an odd number of channels per head, a 1x1 level
    "tail_c6_h2_17x23_r3_l3": ((2, 6, 17, 23, 3, 3, 2), {}),
    "tail_c9_h3_8x64_r1_l4": ((3, 9, 8, 64, 1, 4, 3), dict(seed=1)),
    "tail_c3_h3_7x9_r6_l1": ((1, 3, 7, 9, 6, 1, 3), {}),
    "tail_c1_5x70_r2_l1": ((1, 1, 5, 70, 2, 1, 1), {}),
    "tail_c4_8x8_r3_l4_level3_is_1x1": ((2, 4, 8, 8, 3, 4, 1), {}),
    # h w = 63, 64 (above), 65, 255, 257: around the wavefront and the 256-pixel block
    "hw63_7x9": ((1, 2, 7, 9, 2, 1, 1), {}),
    "hw65_5x13": ((2, 3, 5, 13, 3, 2, 1), {}),
    "hw255_15x17": ((1, 4, 15, 17, 2, 3, 2), {}),
    "hw257_1x257": ((1, 2, 1, 257, 2, 1, 1), {}),
    # LDS bands, L = 1 so the arithmetic is plain
    "lds30k_48x80": ((1, 4, 48, 80, 2, 1, 2), {}),
    "lds50k_64x100": ((1, 4, 64, 100, 2, 1, 1), {}),
    "lds72k_72x128": ((1, 4, 72, 128, 2, 1, 2), {}),
    "lds100k_80x160_odd_c": ((1, 5, 80, 160, 2, 1, 1), {}),
    "lds100k_80x160": ((1, 4, 80, 160, 2, 1, 2), {}),
    "lds168k_96x224": ((1, 4, 96, 224, 2, 1, 2), {}),
    "lds215k_80x256_l3": ((1, 4, 80, 256, 3, 3, 1), dict(seed=2)),
    "dualrefine_like_40x100_r8_l3": ((2, 16, 40, 100, 8, 3, 1), dict(seed=1)),
    # geometry
    "per_sample_K_larger_motion": ((3, 6, 20, 31, 4, 2, 2), dict(k_jitter=0.15, motion=3.0)),
    "third_behind_the_camera": ((2, 4, 24, 40, 3, 2, 1), dict(behind=1.0 / 3)),
    "one_sample_all_outside": ((2, 6, 12, 20, 2, 2, 2), dict(outside=1)),
    "unit_gaussian_cotangents": ((2, 6, 17, 23, 3, 3, 2), dict(heavy=False)),
}
# odd C and heads that split a channel pair: run under each value of the option "epi_bwd_planes"
PLANES_CASES = ("tail_c6_h2_17x23_r3_l3", "tail_c9_h3_8x64_r1_l4", "tail_c3_h3_7x9_r6_l1", "tail_c1_5x70_r2_l1",
                "lds100k_80x160_odd_c")
# cotangent / gradient subsets: one shape on the plane path, one on the atomic path whatever the device's LDS limit
SUBSET_CASES = ("tail_c6_h2_17x23_r3_l3", "lds215k_80x256_l3")
ALIGN_CASES = {  # (B, C, h, w)
    "align_c6_17x23": (2, 6, 17, 23),
    "align_c3_7x9": (1, 3, 7, 9),
    "align_c1_5x70": (1, 1, 5, 70),
    "align_c2_1x257": (1, 2, 1, 257),
    "align_30k_48x80": (1, 4, 48, 80),
    "align_50k_64x100": (1, 4, 64, 100),
    "align_72k_72x128": (1, 4, 72, 128),
    "align_100k_80x160_odd_c": (1, 5, 80, 160),
    "align_168k_96x224": (1, 4, 96, 224),
}
BANDS_KB = ((0, 32), (32, 64), (64, 80), (80, 160), (160, float("inf")))


def lookup_lds_bytes(h, w, L):
    return sum((h >> l) * (w >> l) for l in range(L)) * 8


def align_lds_bytes(h, w):
    return h * w * 8


def band_of(nbytes):
    return next(i for i, (lo, hi) in enumerate(BANDS_KB) if lo * 1024 < nbytes <= hi * 1024)


# ---------------------------------------------------------------- inputs
def heavy_tailed(shape, g):
    """Gaussian x exp(3 Gaussian): real cotangents are heavy-tailed, and the LDS accumulators quantise to the sample's
    largest |cotangent|"""
    return torch.randn(shape, generator=g) * torch.exp(3.0 * torch.randn(shape, generator=g))


def make_sweep_case(B, C, h, w, seed, r=2, L=1, heads=1, k_jitter=0.05, motion=1.0, behind=0.0, outside=None, heavy=True):
    """``oracle.gen_golden_epi.make_case`` plus per-sample intrinsics (fx, cx, cy of sample b perturbed by ``k_jitter``),
    ``motion`` x its rotation and translation, the top ``behind`` share of the rows at depths that the pose's -0.5 forward
    translation puts behind the camera (1/Z < 0; and the clamp at 100 bites next to it), sample ``outside`` translated so
    that every hypothesis projects far outside the image, and the three cotangents (``heavy``: heavy-tailed w_corr)."""
    K, depth, poses, f1, f2 = make_case(B, C, h, w, seed)
    g = torch.Generator().manual_seed(seed + 9000)
    K = K.clone()
    K[:, 0, 0] *= 1.0 + k_jitter * (2 * torch.rand(B, generator=g) - 1)
    K[:, 0, 2] += k_jitter * w * (2 * torch.rand(B, generator=g) - 1)
    K[:, 1, 2] += k_jitter * h * (2 * torch.rand(B, generator=g) - 1)
    if motion != 1.0:
        poses = poses.clone()
        poses[:, :3, 3] *= motion
        ang = motion * 0.02 * torch.randn(B, generator=g)
        poses[:, 0, 0], poses[:, 0, 2], poses[:, 2, 0], poses[:, 2, 2] = torch.cos(ang), torch.sin(ang), -torch.sin(ang), torch.cos(ang)
    if behind > 0:
        rows = max(1, int(round(behind * h)))
        depth = depth.clone()
        depth[:, :, :rows] = 0.15 + 0.2 * (depth[:, :, :rows] - 1.0) / 8.0
        # the next row's nearest hypothesis (depth x (1 - softplus(delta) 2^(L-1) / 8)) at 0 < Z < 0.01: the clamp at 100.
        # No rotation, so that Z = depth - 0.5 and no hypothesis lands at a tiny NEGATIVE Z, where 1/Z is unclamped and
        # the coordinate's conditioning is 1/|Z|
        lo = 1.0 - float(torch.nn.functional.softplus(torch.tensor(DELTA))) * 2 ** (L - 1) / 8.0
        depth[:, :, rows] = torch.linspace(0.501, 0.509, w) / lo
        poses = poses.clone()
        poses[:, :3, :3] = torch.eye(3)
        poses[:, 2, 3] = -0.5
    if outside is not None:
        poses = poses.clone()
        poses[outside, 0, 3] = 500.0
    D = L * (2 * r + 1)
    w_corr = heavy_tailed((B, D * heads, h, w), g) if heavy else torch.randn(B, D * heads, h, w, generator=g)
    w_ds, w_mx = 0.1 * torch.randn(B, 1, D, h, w, generator=g), torch.randn(B, 1, h, w, generator=g)
    return dict(K=K, depth=depth.contiguous(), poses=poses, f1=f1, f2=f2, delta=torch.tensor([DELTA]), r=r, L=L, heads=heads,
                w_corr=w_corr, w_ds=w_ds, w_mx=w_mx)


def lookup_case(name):
    (B, C, h, w, r, L, heads), opts = LOOKUP_CASES[name]
    opts = dict(opts)
    seed = _seed_of(name) + opts.pop("seed", 0)
    return make_sweep_case(B, C, h, w, seed, r=r, L=L, heads=heads, **opts)


def _seed_of(name):
    return zlib.crc32(name.encode()) % 10000


def align_case(name):
    """the inputs of the align case ``name``, seeded by the name like ``lookup_case``"""
    return make_align_case(*ALIGN_CASES[name], seed=_seed_of(name))


def make_align_case(B, C, h, w, seed):
    """inputs of the pose-refinement step: a target that resembles the source (a well-conditioned step), per-sample K"""
    c = make_sweep_case(B, C, h, w, seed, k_jitter=0.05)
    K, depth, f1 = c["K"], c["depth"], c["f1"]
    poses = make_case(B, C, h, w, seed, trans=0.05)[2]
    g = torch.Generator().manual_seed(seed + 77)
    i = dict(K=K, depth=depth, poses=poses, f1=f1, f2=(0.8 * f1 + 0.2 * c["f2"]).half().float())
    for k in ("src_w", "tgt_w", "weight"):
        i[k] = 0.5 + torch.rand(B, 1, h, w, generator=g)
    return i


# ---------------------------------------------------------------- references
def _cast(c, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in c.items()}


def oracle_lookup(c, dtype, terms=("corr", "ds", "max_dx"), need=LEAVES):
    """the oracle's outputs and the gradients of sum over ``terms`` of <output, cotangent> w.r.t. ``need``, in ``dtype``"""
    c = _cast(c, dtype)
    lv = {k: c[k].clone().requires_grad_(k in need) for k in LEAVES}
    coords, max_dx, ds = E.depth2epipolarcoords(lv["poses"], lv["depth"], c["K"], lv["delta"], r=c["r"], num_levels=c["L"])
    corr = E.coord_sample(lv["f1"], E.pyramid(lv["f2"], c["L"]), coords, c["L"], c["heads"])
    out = dict(coords=coords.detach(), max_dx=max_dx.detach(), ds=ds.detach(), corr=corr.detach())
    s = 0
    for t, o, wt in (("corr", corr, c["w_corr"]), ("ds", ds, c["w_ds"]), ("max_dx", max_dx, c["w_mx"])):
        if t in terms:
            s = s + (o * wt).sum()
    s.backward()
    return out, {k: v.grad for k, v in lv.items() if k in need}


def reference(c, **kw):
    """-> (outputs, gradients) of the oracle in fp64 and (outputs, gradients) in fp32"""
    return oracle_lookup(c, torch.float64, **kw), oracle_lookup(c, torch.float32, **kw)


# ---------------------------------------------------------------- the gate
def distance(x, ref64):
    """max |x - ref64| relative to ref64's largest magnitude (absolute where that is zero)"""
    sc = float(ref64.abs().max())
    return float((x.double() - ref64).abs().max()) / sc if sc > 0 else float((x.double() - ref64).abs().max())


def check(got, ref64, ref32, numel=None, forward=False, floor=1e-4, what=""):
    """dicts of tensors by name.  ``forward``: no allowance on any tensor.  The allowance's 4/numel term uses the larger of
    the tensor's own element count (as ``check_grads`` does) and ``numel``: passing it can only tighten.  ``ref32`` None is
    ``admissible``'s form, the fp32 oracle against fixed floors: ``floor`` on forward values and per-pixel maps,
    ``SUM_FLOOR`` on the few-element gradients (see ``admissible``).  Returns the figures."""
    report = {}
    for k, r in ref64.items():
        if r is None:
            assert got[k] is None or not got[k].abs().max() > 0, (what, k)
            continue
        g = got[k].reshape(r.shape).double()
        fin = torch.isfinite(r)
        if not fin.all():  # the clamp at 100 never yields them; if it did: the same elements non-finite, the finite ones held
            assert torch.equal(torch.isfinite(g), fin), (what, k)
            g, r = torch.where(fin, g, torch.zeros_like(g)), torch.where(fin, r, torch.zeros_like(r))
            if ref32 is not None:
                ref32 = dict(ref32)
                ref32[k] = torch.where(fin, ref32[k].reshape(r.shape).double(), torch.zeros_like(r))
        sc = float(r.abs().max())
        small = g.numel() <= 64
        if ref32 is None:
            tol = SUM_FLOOR if (small and not forward) else floor
        else:
            tol = max(floor, 1.25 * distance(ref32[k].reshape(r.shape), r))
        d = (g - r).abs()
        if forward or small:
            report[k] = (float(d.max()) / max(sc, 1e-30), tol)
            assert float(d.max()) <= tol * sc + 1e-30, (what, k, float(d.max()), sc, tol)
        else:
            bad = float((d > tol * sc).double().mean())
            l2 = float(np.linalg.norm(d.numpy().ravel()) / (np.linalg.norm(r.numpy().ravel()) + 1e-300))
            cap = 2e-4 + 4.0 / max(g.numel(), numel or 0)
            report[k] = (float(d.max()) / max(sc, 1e-30), tol, bad, cap, l2)
            assert bad <= cap, (what, k, bad, cap, float(d.max()), sc, tol)
            assert l2 <= 2e-3, (what, k, l2)
    return report


def admissible(ref64, ref32, forward=False, what=""):
    """the condition on a case: the fp32 oracle alone is inside the gate at its floor -- forward values within 1e-4, per-pixel
    maps within the allowance at 1e-4.  The few-element gradients (poses, delta: sums over every pixel and hypothesis of
    heavy-tailed terms) are gated at 1.25 x the fp32 oracle's distance, which is only a test of the kernel while that
    distance is rounding and not cancellation.  Two correct fp32 summations of the same terms differ from each other by
    small multiples of that distance, so the fp32 oracle must be within a quarter of the floor (2.5e-5; it is at 1e-7 to
    2e-5 on unexceptional inputs): inputs whose heavy tail puts one dominant term on a sensitive pixel (the oracle at
    2e-4 to 4e-4) are refused and replaced by the next seed (``seed`` in the table)."""
    return check(ref32, ref64, None, forward=forward, what=what)


# ---------------------------------------------------------------- the device
def _args(r, L, robust=False):
    return SimpleNamespace(corr_radius=r, disable_pose_updates=False, gap_factor="depth", gap_factor_depth_ratio=8, num_levels=L,
                           disable_fixed_pose_weight=True, robust_pose_loss=robust)


def run_lookup(c, terms=("corr", "ds", "max_dx"), need=LEAVES):
    """``mal_amd.epipolar``'s public objects on the device -> (outputs, gradients; None for a leaf outside ``need``)"""
    from mal_amd import epipolar
    d = lambda t: t.to(DEV)
    R = epipolar.Reprojections(_args(c["r"], c["L"])).to(DEV)
    with torch.no_grad():
        R.delta.fill_(float(c["delta"]))
    R.delta.requires_grad_("delta" in need)
    R._reg_intrinsics(d(c["K"]))
    lv = {k: d(c[k]).clone().requires_grad_(k in need) for k in ("depth", "poses", "f1", "f2")}
    coords, max_dx, ds = R.depth2epipolarcoords(lv["poses"], lv["depth"])
    S = epipolar.CoordSampler(_args(c["r"], c["L"]))
    S.register(lv["f1"], lv["f2"], num_levels=c["L"])
    corr = S(coords, c["L"], c["heads"])
    out = {k: v.detach().cpu() for k, v in dict(coords=coords, max_dx=max_dx, ds=ds, corr=corr).items()}
    s = 0
    for t, o, wt in (("corr", corr, c["w_corr"]), ("ds", ds, c["w_ds"]), ("max_dx", max_dx, c["w_mx"])):
        if t in terms:
            s = s + (o * d(wt)).sum()
    if need:
        s.backward()
    torch.cuda.synchronize()
    lv["delta"] = R.delta
    return out, {k: (None if v.grad is None else v.grad.cpu()) for k, v in lv.items()}


# ---------------------------------------------------------------- the corner table (csrc/mal_sample.h)
# The lookup takes its coordinates as an input, so sampling positions can be placed exactly: h and w are powers of two, one
# level, so the position in elements IS the coordinate (2 (x + 0.5) / 8 - 1 and back are exact).  x runs along the hypothesis
# axis, one call per y: on and next to every bound of the corner code -- the first and last column / row, -1 and size (the
# outermost floor with no tap inside), one float inside them, far outside (the clamp of the int conversion).
CORNER_SHAPE = (1, 4, 4, 8)  # B, C, h, w; one level, one head
CORNER_X = (-1.5, -1.0, -0.5, -2.0 ** -20, 0.0, 0.25, 3.0, 6.5, 7.0, 7.0 + 2.0 ** -20, 7.5, 8.0, 1e4, -1e4, 1e30)
CORNER_Y = (-1.5, -1.0, -0.5, 0.0, 1.5, 3.0, 3.5, 4.0, 1e30)
CORNER_WILD_X = (float("nan"), float("inf"))  # held to the all-padding property only, not to the oracle


def all_padding(x, y):
    """every tap of the position is padding or carries a weight of exactly zero: the sample is 0 and nothing reaches fmap2"""
    B, C, h, w = CORNER_SHAPE
    return x != x or y != y or x <= -1 or x >= w or y <= -1 or y >= h


def corner_case(y, xs=CORNER_X):
    """-> f1, f2 (fp16-representable), coords (1,2,1,len(xs),h,w) with x = xs[j] and y everywhere, a cotangent that is
    non-zero on the all-padding hypotheses only, and a cotangent that is non-zero everywhere"""
    B, C, h, w = CORNER_SHAPE
    g = torch.Generator().manual_seed(4242)
    f1, f2 = (torch.randn(B, C, h, w, generator=g).half().float() for _ in range(2))
    coords = torch.empty(B, 2, 1, len(xs), h, w)
    coords[:, 0, 0] = torch.tensor(xs, dtype=torch.float32)[None, :, None, None]
    coords[:, 1, 0] = y
    w_all = 0.5 + torch.rand(B, len(xs), h, w, generator=g)
    pad = torch.tensor([all_padding(x, y) for x in xs])
    return dict(f1=f1, f2=f2, coords=coords, pad=pad, w_pad=w_all * pad[None, :, None, None], w_all=w_all)


def corner_oracle(c, dtype, cot="w_all"):
    """-> (corr, d <corr, cotangent> / d f2) of oracle.epi_oracle.coord_sample in ``dtype``"""
    f2 = c["f2"].to(dtype).clone().requires_grad_(True)
    corr = E.coord_sample(c["f1"].to(dtype), [f2], c["coords"].to(dtype), 1, 1)
    (corr * c[cot].to(dtype)).sum().backward()
    return corr.detach(), f2.grad


def mean_abs_f1(c):
    """mean |fmap1| over the four channels as the kernel sums them: in channel order, in fp32 (exact here: fp16 inputs)"""
    a = c["f1"].abs()
    return (((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]) * 0.25


def run_corner(c, cot):
    """the device's lookup at the case's coordinates -> (corr, d <corr, c[cot]> / d f2)"""
    from mal_amd import epipolar
    d = lambda t: t.to(DEV)
    f2 = d(c["f2"]).clone().requires_grad_(True)
    S = epipolar.CoordSampler(_args(2, 1))
    S.register(d(c["f1"]), f2, num_levels=1)
    corr = S(d(c["coords"]), 1, 1)
    (corr * d(c[cot])).sum().backward()
    torch.cuda.synchronize()
    return corr.detach().cpu(), f2.grad.cpu()


# ---------------------------------------------------------------- pose refinement, piecewise
def oracle_gradcoords(i, dtype, w_cp=None, w_P2=None):
    """depth2gradcoords and the gradients of <c_p, w_cp> + <P2, w_P2> (either may be None) w.r.t. depth and poses"""
    lv = dict(depth=i["depth"].to(dtype).clone().requires_grad_(True), poses=i["poses"].to(dtype).clone().requires_grad_(True))
    c_p, P2 = E.depth2gradcoords(lv["poses"], lv["depth"], i["K"].to(dtype))
    s = 0
    if w_cp is not None:
        s = s + (c_p * w_cp.to(dtype)).sum()
    if w_P2 is not None:
        s = s + (P2 * w_P2.to(dtype)).sum()
    s.backward()
    return dict(c_p=c_p.detach(), P2=P2.detach()), {k: v.grad for k, v in lv.items()}


NEQ_LEAVES = ("f1", "f2", "src_w", "tgt_w", "weight", "p2", "P2")


def oracle_normal_eq(i, p2, P2, dtype, g_H, g_b, robust, use_weight=True, need=NEQ_LEAVES):
    v = dict(i, p2=p2, P2=P2)
    names = [k for k in NEQ_LEAVES if use_weight or k != "weight"]
    lv = {k: v[k].to(dtype).clone().requires_grad_(k in need) for k in names}
    H, b = E.normal_equations(lv["f1"], lv["f2"], lv["src_w"], lv["tgt_w"], i["K"].to(dtype), lv["p2"], lv["P2"],
                              lv.get("weight"), robust=robust)
    ((H * g_H.to(dtype)).sum() + (b * g_b.to(dtype)).sum()).backward()
    return dict(H=H.detach(), b=b.detach()), {k: t.grad for k, t in lv.items() if k in need}


def run_gradcoords(i, w_cp=None, w_P2=None):
    from mal_amd import epipolar
    d = lambda t: t.to(DEV)
    R = epipolar.Reprojections(_args(2, 1)).to(DEV)
    R._reg_intrinsics(d(i["K"]))
    lv = dict(depth=d(i["depth"]).clone().requires_grad_(True), poses=d(i["poses"]).clone().requires_grad_(True))
    c_p, P2 = R.depth2gradcoords(lv["poses"], lv["depth"], d(i["K"]))
    s = 0
    if w_cp is not None:
        s = s + (c_p * d(w_cp)).sum()
    if w_P2 is not None:
        s = s + (P2 * d(w_P2)).sum()
    s.backward()
    torch.cuda.synchronize()
    return dict(c_p=c_p.detach().cpu(), P2=P2.detach().cpu()), {k: v.grad.cpu() for k, v in lv.items()}


def run_normal_eq(i, p2, P2, g_H, g_b, robust, use_weight=True, need=NEQ_LEAVES):
    from mal_amd import epipolar
    d = lambda t: t.to(DEV)
    v = dict(i, p2=p2, P2=P2)
    names = [k for k in NEQ_LEAVES if use_weight or k != "weight"]
    lv = {k: d(v[k]).clone().requires_grad_(k in need) for k in names}
    P = epipolar.PoseUpdate(_args(2, 1, robust))
    P.compute_feat(lv["f1"], lv["f2"])
    P.src_w, P.tgt_w = lv["src_w"], lv["tgt_w"]
    H, b = P.normal_equations(d(i["K"]), lv["p2"], lv["P2"], lv.get("weight"))
    ((H * d(g_H)).sum() + (b * d(g_b)).sum()).backward()
    torch.cuda.synchronize()
    return dict(H=H.detach().cpu(), b=b.detach().cpu()), {k: (None if t.grad is None else t.grad.cpu()) for k, t in lv.items()}


def on_the_robust_bounds(p2):
    """a copy of p2 (B,2,1,5,h,w) with the first pixels' stencils moved so that the centre lies exactly ON the in-image
    test's bounds 2 and w-3 / h-3 (inside: the test is inclusive) and one float below / above them (outside), and the
    (h,w) mask of the moved pixels.  Their stencils lie on integer positions, i.e. ON tap boundaries, where the slope
    w.r.t. the position is one-sided and the side is picked by the rounding of the unnormalised coordinate: d/d p2 is
    compared outside the mask; everything else (H, b and the other gradients are continuous there) everywhere."""
    p2 = p2.clone()
    moved = torch.zeros(p2.shape[-2:], dtype=torch.bool)
    h, w = p2.shape[-2:]
    f = lambda v: float(np.float32(v))
    below, above = f(np.nextafter(np.float32(2.0), np.float32(0.0))), f(np.nextafter(np.float32(w - 3), np.float32(w)))
    xs = [2.0, float(w - 3), below, above]
    for n, x in enumerate(xs):
        if n >= h * w:
            break
        yy, xx = divmod(n, w)
        moved[yy, xx] = True
        y = float(p2[0, 1, 0, 0, yy, xx])
        p2[0, 0, 0, :, yy, xx] = torch.tensor([x, f(x + 1), f(x - 1), x, x])
        p2[0, 1, 0, :, yy, xx] = torch.tensor([y, y, y, f(y + 1), f(y - 1)])
    if h >= 7:
        for n, y in enumerate([2.0, float(h - 3)]):
            yy, xx = divmod(len(xs) + n, w)
            moved[yy, xx] = True
            x = min(max(float(p2[0, 0, 0, 0, yy, xx]), 3.0), w - 4.0)
            p2[0, 0, 0, :, yy, xx] = torch.tensor([x, f(x + 1), f(x - 1), x, x])
            p2[0, 1, 0, :, yy, xx] = torch.tensor([y, y, y, f(y + 1), f(y - 1)])
    return p2, moved


def robust_rejects(p2):
    """(row, column) of sample 0's moved pixels that lie one float OUTSIDE the robust mask's bounds: their weight is exactly
    zero, so under ``--robust_pose_loss`` nothing they touch receives a gradient and d/d p2 there is exactly zero"""
    h, w = p2.shape[-2:]
    return [divmod(n, w) for n in (2, 3) if n < h * w]


def outside_mask(grads, moved):
    """the gradients with d/d p2 zeroed at sample 0's moved pixels"""
    g = dict(grads)
    if g.get("p2") is not None:
        g["p2"] = g["p2"].clone()
        g["p2"][0][..., moved] = 0
    return g


def solve_admissible(H):
    """the solve's gate is 2e-3 per sample, "the normal equations' error times the conditioning": with fp32's 6e-8 that is a
    statement about the kernel up to a condition number of about 1e4 (6e-4, a third of the gate).  An image one pixel high
    has no y-gradient and a near-singular H (1e9): its solve is not held, its other pieces are."""
    return bool((torch.linalg.cond(H.double()) <= 1e4).all())


# ---------------------------------------------------------------- the solver's three outcomes
def crafted_systems():
    """-> (H (6,6,6), b (6,6), poses (6,4,4), the branch each row must take): symmetric positive definite rows, a symmetric
    indefinite non-singular one (Cholesky fails, LU solves), one whose first row and column are exactly zero (both fail)
    and one holding a NaN (both fail), interleaved so that every failing row has healthy neighbours"""
    g = torch.Generator().manual_seed(5)
    spd = []
    for _ in range(3):
        A = torch.randn(6, 6, generator=g)
        spd.append(A @ A.T + 6 * torch.eye(6))
    Q = torch.linalg.qr(torch.randn(6, 6, generator=g))[0]
    indef = Q @ torch.diag(torch.tensor([3.0, -2.0, 1.5, -1.0, 2.5, 0.7])) @ Q.T
    indef = 0.5 * (indef + indef.T)
    sing = spd[0].clone()
    sing[0, :], sing[:, 0] = 0.0, 0.0
    nan = spd[1].clone()
    nan[2, 3] = nan[3, 2] = float("nan")
    H = torch.stack([spd[0], indef, spd[1], sing, nan, spd[2]])
    b = torch.randn(6, 6, generator=g)
    poses = make_case(6, 1, 4, 4, 21)[2]
    return H, b, poses, [E.CHOLESKY, E.LU, E.CHOLESKY, E.FAILED, E.FAILED, E.CHOLESKY]


def oracle_update(H, b, poses, dtype, g_new, g_up):
    """``align_update_per_sample`` and the gradients of <new, g_new> + <update, g_up> (either may be None); a failed row
    sends nothing to H / b: zeros"""
    lv = dict(H=H.to(dtype).clone().requires_grad_(True), b=b.to(dtype).clone().requires_grad_(True),
              poses=poses.to(dtype).clone().requires_grad_(True))
    new, up, branches = E.align_update_per_sample(lv["H"], lv["b"], lv["poses"])
    s = 0
    if g_new is not None:
        s = s + (new * g_new.to(dtype)).sum()
    if g_up is not None:
        s = s + (up * g_up.to(dtype)).sum()
    s.backward()
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in lv.items()}
    return dict(new=new.detach(), update=up.detach()), grads, branches


def run_update(H, b, poses, g_new, g_up):
    from mal_amd import epipolar
    d = lambda t: t.to(DEV)
    lv = dict(H=d(H).clone().requires_grad_(True), b=d(b).clone().requires_grad_(True), poses=d(poses).clone().requires_grad_(True))
    new, up = epipolar.AlignUpdateFn.apply(lv["H"], lv["b"], lv["poses"])
    s = 0
    if g_new is not None:
        s = s + (new * d(g_new)).sum()
    if g_up is not None:
        s = s + (up * d(g_up)).sum()
    s.backward()
    torch.cuda.synchronize()
    return dict(new=new.detach().cpu(), update=up.detach().cpu()), {k: v.grad.cpu() for k, v in lv.items()}
