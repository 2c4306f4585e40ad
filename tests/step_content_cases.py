"""Case table of the content sweep of the one-call loss steps (tests/test_step_content_cases.py on the CPU,
tests/test_gpu_step_content_sweep.py on the device).

Every other whole-step test draws its batch from mal_amd.synthetic.make_batch: one K for the whole batch, tiny motion,
mid-range disparities, textured images, random masks.  The builders here take such a batch and return one of the same
contract whose CONTENT reaches what the marching kernels restate for themselves: the per-sample camera block, the border
clamp and the clipped-sample masks, the guarded division behind the camera, both ends of the depth range, SSIM on its clamp
with every L1 sign at 0, and the `x / (0 + 1e-7)` tails of a sample or a batch without one live student weight.

Pure CPU; every case draws from a private torch.Generator seeded from its name and shape.
"""
import zlib

import numpy as np
import torch

from mal_amd.synthetic import make_batch
from oracle import mal_oracle as O

SHAPES = ((2, 24, 72), (3, 37, 50))       # two strips / three row segments; ragged; B >= 2 so that a wrong sample index shows
MS_SHAPE = (3, 40, 72)                    # the four-scale step (sclm 2)
DR_SHAPE = (2, 40, 72)                    # the DualRefine step (scales [0], n_losses 1)
GEOMETRY = ("per_sample_K", "large_motion", "behind_camera")
MS_GEOMETRY = ("per_sample_K", "large_motion", "behind_camera_whole_samples")  # (see behind_camera_whole_samples)
MS_SCLM = 2
DEAD = ("dead_weights_one_sample", "dead_weights_all")
VARIANTS = GEOMETRY + ("disp_extremes", "flat_images") + DEAD
MIN_DEPTH, MAX_DEPTH = 0.1, 100.0         # oracle.mal_oracle.default_opt
# Seeds.  Every condition of tests/test_step_content_cases.py is met ON THE ORACLE ALONE; where the first seed tried did not
# meet one, another was taken (never a wider condition):
#  - make_batch's seed is 4000, except
#    (3, 37, 50): 4008.  make_batch(3, 37, 50, seed=4000) has 11 pixels in disp_student (12 in 0.3 x disp_teacher) whose
#      neighbour is within a few ulp: the sign of the RAW difference, which the kernels take, and of the difference of the
#      normalised maps, which the oracle takes, differ there -- near-ties all, but more than the gate's 3e-4 N + 8 = 9.7.
#      Seed 4008 has 4 and 3 (2 and 0);
#    `large_motion` elsewhere: 4002 (4000 puts 0.25 / 0.26 of frame +1's samples of (2, 24, 72) outside, on the band's edge);
#  - SALTS: a further draw of the case's own generator.  The poses of `large_motion` come from it ((3, 40, 72): frame +1 at
#    0.21 without); so do the factors of `per_sample_K`, whose control moves the loss by 1.5e-3 / 1.3e-3 without and by
#    2.9e-3 / 5.7e-3 with (condition: > 1e-3).
DEFAULT_SEED = 4000
SHAPE_SEEDS = {(3, 37, 50): 4008}
SEEDS = {("large_motion", s): 4002 for s in ((2, 24, 72), MS_SHAPE, DR_SHAPE)}
SALTS = {("large_motion", MS_SHAPE): 4, ("per_sample_K", (2, 24, 72)): 1, ("per_sample_K", (3, 37, 50)): 1}
MOTION = (0.05, 0.25)  # `large_motion`: axis-angle and translation as multiples of N(0, 1)
# leaves on which the fp32 forced oracle ITSELF is further than 8e-5 (L2 rel) from the fp64 one (the table of
# tests/test_step_content_cases.py): the device test keeps the checker's max(1e-4, 1.25 x floor) there and
# plain 1e-4 on every other leaf of every case
FLOOR_LEAVES = {("flat_images", (2, 24, 72)): ("translation_m1",)}


def _gen(name, shape):
    if name in DEAD:  # the same draws as `base`: a dead-weight case differs from the base batch by its edit of the masks alone
        name = "base"
    salt = SALTS.get((name, tuple(shape)), 0)
    return torch.Generator().manual_seed(zlib.crc32(("%s/%dx%dx%d" % ((name,) + tuple(shape)) + "/%d" % salt * bool(salt)).encode()))


def seed_of(name, shape):
    return SEEDS.get((name, tuple(shape)), SHAPE_SEEDS.get(tuple(shape), DEFAULT_SEED))


def base(b, g):
    """make_batch's content with masks that bite: make_batch(2, 24, 72, seed=4000) sets both augmentation flags, every student
    weight is then zero and no mask changes anything -- so augmentation is off everywhere and the consistency mask is drawn here"""
    b = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}
    B, _, H, W = b["color0"].shape
    b["augmentation_mask"] = torch.zeros(B, 1, 1, 1)
    b["consistency_mask"] = (torch.rand(B, H, W, generator=g) < 0.8).float()
    return b


def per_sample_K(b, g, jitter=0.1):
    """fx, fy, cx, cy of every sample scaled by independent factors in [1 - jitter, 1 + jitter]; inv_K = pinv(K) in float64, cast
    (mal_amd.synthetic.kitti_intrinsics does the same for its one matrix)"""
    b = base(b, g)
    B = b["K"].shape[0]
    K = b["K"].double().clone()
    f = 1 + jitter * (2 * torch.rand(B, 4, generator=g, dtype=torch.float64) - 1)
    K[:, 0, 0] *= f[:, 0]
    K[:, 1, 1] *= f[:, 1]
    K[:, 0, 2] *= f[:, 2]
    K[:, 1, 2] *= f[:, 3]
    b["K"] = K.float().contiguous()
    b["inv_K"] = torch.from_numpy(np.stack([np.linalg.pinv(k) for k in b["K"].double().numpy()])).float().contiguous()
    return b


def broadcast_K0(b):
    """the control of per_sample_K: what a kernel that read `K + 0` would have computed"""
    b = dict(b)
    B = b["K"].shape[0]
    b["K"] = b["K"][:1].repeat(B, 1, 1).contiguous()
    b["inv_K"] = b["inv_K"][:1].repeat(B, 1, 1).contiguous()
    return b


def large_motion(b, g):
    b = per_sample_K(b, g)
    B, _, H, W = b["color0"].shape
    aa, tr = MOTION
    for s in ("m1", "p1"):
        b["axisangle_" + s] = aa * torch.randn(B, 1, 3, generator=g)
        b["translation_" + s] = tr * torch.randn(B, 1, 3, generator=g)
    return b


NEAR_DISP = (0.9, 1.0)  # depth 1 / (0.01 + 9.99 d): 0.1112 ... 0.1
FAR_SCALE = 0.3         # everywhere else make_batch's disparities (< 0.55) are scaled to < 0.165: depth > 0.6, z' > 0.1


def behind_camera(b, g):
    """t_z = +0.5 for frame -1 (its pose is inverted: the points move by -0.5 in z) and -0.5 for frame +1; the top third of the
    teacher's rows and the bottom-left quarter of the student's at depth 0.1 ... 0.112: z' < 0 there.  Everything else is moved
    AWAY from z' = 0 (depth 0.5): the rest of both maps is scaled by FAR_SCALE, so |z'| >= 1e-3 holds by construction and not by
    the luck of a seed (an exact division by zero and ATen's NaN grid are no reference)."""
    b = base(b, g)
    B, _, H, W = b["color0"].shape
    b["translation_m1"] = b["translation_m1"].clone()
    b["translation_p1"] = b["translation_p1"].clone()
    b["translation_m1"][:, 0, 2] = 0.5
    b["translation_p1"][:, 0, 2] = -0.5
    lo, hi = NEAR_DISP
    for k in ("disp_teacher", "disp_student"):
        b[k] = (b[k] * FAR_SCALE).contiguous()
    b["disp_teacher"][:, :, :H // 3, :] = lo + (hi - lo) * torch.rand(B, 1, H // 3, W, generator=g)
    b["disp_student"][:, :, H - H // 2:, :W // 2] = lo + (hi - lo) * torch.rand(B, 1, H // 2, W // 2, generator=g)
    return b


def behind_camera_whole_samples(b, g):
    """behind_camera for the four-scale step.  Its lower scales are pooled copies, upsampled again: across the border of a near
    region inside one image the upsampled disparity takes every value between near and far, z' = 0 among them (measured with
    the rows / quarter layout at (3, 40, 72): min |z'| 1.4e-4 at scale 2).  So here whole samples are near -- the teacher's map
    of sample 0, the student's of sample 1 -- and pooling, which never mixes samples, keeps every scale away from z' = 0."""
    b = base(b, g)
    B, _, H, W = b["color0"].shape
    b["translation_m1"] = b["translation_m1"].clone()
    b["translation_p1"] = b["translation_p1"].clone()
    b["translation_m1"][:, 0, 2] = 0.5
    b["translation_p1"][:, 0, 2] = -0.5
    lo, hi = NEAR_DISP
    for k in ("disp_teacher", "disp_student"):
        b[k] = (b[k] * FAR_SCALE).contiguous()
    b["disp_teacher"][0] = lo + (hi - lo) * torch.rand(1, H, W, generator=g)
    b["disp_student"][1] = lo + (hi - lo) * torch.rand(1, H, W, generator=g)
    return b


def disp_extremes(b, g):
    b = base(b, g)
    b["disp_teacher"][:, :, :4, :] = 0.0
    b["disp_teacher"][:, :, -4:, :] = 1.0
    b["disp_student"][:, :, :, :5] = 1.0
    b["disp_student"][:, :, :, -5:] = 0.0
    return b


FLAT_VALUE = 0.0


def flat_images(b, g, value=None):
    """sample 0: all three images exactly 0; sample 1: the left half of all three exactly FLAT_VALUE, a flat / textured border
    inside one sample.  SSIM's pre-clamp term is exactly 0 there and every L1 sign is 0.

    The flat value of sample 1 is 0 and not 1: a bilinear warp of a constant c is c x (the sum of four rounded weights), exact
    for c = 0 only.  With 1.0 both candidates of a flat pixel are 0 in exact arithmetic and 0 or 9e-9 in fp32 as the weights
    happen to round, so two correct evaluations break that tie differently at some 3 % of the flat pixels: the fp32 oracle
    against the fp64 oracle differs in `win_t` at 12-41 pixels of (2, 24, 72) over twelve seeds (cap 9.0; `win_s` 6-38) and at
    5-37 of (3, 37, 50) (cap 9.7): the reference alone does not meet the count cap on that content."""
    b = base(b, g)
    W = b["color0"].shape[-1]
    for k in ("color0", "color_m1", "color_p1"):
        b[k][0] = 0.0
        b[k][1, :, :, :W // 2] = FLAT_VALUE if value is None else value
    return b


DEAD_COST = 1e-3  # a cost-volume disparity of 1e-3 is a depth of 1000: ten times max_depth, the matching mask is false


def dead_weights_one_sample(b, g):
    b = base(b, g)
    b["consistency_mask"][0] = 0.0
    b["lowest_cost"][-1] = DEAD_COST
    return b


def dead_weights_all(b, g):
    """every student weight dead, through the consistency mask (even samples), the matching mask (odd samples), and -- the last
    sample of an odd batch -- the consistency mask on the top half and the matching mask on the rest.  Augmentation stays 0: the
    augmented-sample skip is not what zeroes them."""
    b = base(b, g)
    B, _, H, W = b["color0"].shape
    for i in range(B):
        if i == B - 1 and B % 2 == 1:
            b["consistency_mask"][i, :H // 2] = 0.0
            b["lowest_cost"][i, H // 2:] = DEAD_COST
        elif i % 2 == 0:
            b["consistency_mask"][i] = 0.0
        else:
            b["lowest_cost"][i] = DEAD_COST
    return b


BUILDERS = dict(base=base, per_sample_K=per_sample_K, large_motion=large_motion, behind_camera=behind_camera,
                behind_camera_whole_samples=behind_camera_whole_samples,
                disp_extremes=disp_extremes, flat_images=flat_images, dead_weights_one_sample=dead_weights_one_sample,
                dead_weights_all=dead_weights_all)
_CACHE = {}


def case(name, shape, with_syn=False):
    """(batch, n0, n1) of one (variant, shape): built once and shared; the tests leave it unchanged"""
    key = (name, tuple(shape), bool(with_syn))
    if key not in _CACHE:
        B, H, W = shape
        g = _gen(name, shape)
        b = BUILDERS[name](make_batch(B, H, W, seed=seed_of(name, shape), with_syn=with_syn), g)
        n0, n1 = torch.randn(B, 1, H, W, generator=g), torch.randn(B, 1, H, W, generator=g)
        _CACHE[key] = (b, n0, n1)
    return _CACHE[key]


# ------------------------------------------------------------------ what the fp64 oracle says of a case's edge
def to64(b):
    return {k: (v.double() if torch.is_tensor(v) and v.dtype == torch.float32 else v) for k, v in b.items()}


def projected_z(b, who):
    """z' = z + 1e-7 of project_3d for both frames, (B,2,H,W), in the batch's own precision (manydepth/layers.py:184-199)"""
    B, _, H, W = b["color0"].shape
    _, depth = O.disp_to_depth(b["disp_teacher" if who == "teacher" else "disp_student"], MIN_DEPTH, MAX_DEPTH)
    pts = O.backproject_depth(depth, b["inv_K"])
    out = []
    for s, inv in (("m1", True), ("p1", False)):
        T = O.transformation_from_parameters(b["axisangle_" + s], b["translation_" + s], inv)
        cam = torch.matmul(torch.matmul(b["K"], T)[:, :3, :], pts)
        out.append(cam[:, 2].view(B, H, W) + 1e-7)
    return torch.stack(out, 1)


def clipped_share(sample):
    """per frame: the share of sampling positions with |grid| >= 1 in either axis (grid_sample's border clamp acts there)"""
    return {f: float((np.abs(sample[f]) >= 1).any(-1).mean()) for f in (-1, 1)}


def ssim_preclamp(x, y):
    """(1 - n / d) / 2 of oracle.mal_oracle.ssim before its clamp to [0, 1]"""
    import torch.nn.functional as F
    xp, yp = F.pad(x, (1, 1, 1, 1), mode="reflect"), F.pad(y, (1, 1, 1, 1), mode="reflect")
    pool = lambda t: F.avg_pool2d(t, 3, 1)
    mu_x, mu_y = pool(xp), pool(yp)
    sig_x, sig_y, sig_xy = pool(xp ** 2) - mu_x ** 2, pool(yp ** 2) - mu_y ** 2, pool(xp * yp) - mu_x * mu_y
    n = (2 * mu_x * mu_y + O.SSIM_C1) * (2 * sig_xy + O.SSIM_C2)
    d = (mu_x ** 2 + mu_y ** 2 + O.SSIM_C1) * (sig_x + sig_y + O.SSIM_C2)
    return (1 - n / d) / 2


def student_weight_sums(o):
    """per sample: the sum of consistency x matching x (1 - augmentation) as the oracle formed it (augmentation is 0 in every case)"""
    return o["consistency_mask"].reshape(o["consistency_mask"].shape[0], -1).sum(1)
