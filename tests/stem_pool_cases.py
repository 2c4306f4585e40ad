"""The case table of the stem max-pool (mal_amd.glue.stem_pool, mal_amd/csrc/mal_pool.hip), importable without a device.
Shared by tests/test_stem_pool_cases.py (CPU: the restatement against torch) and tests/test_gpu_stem_pool.py (GPU).

A case is (shape, filling).  Shapes: the smallest planes (every way a window is clipped), odd and even sizes, widths either
side of a wave's (64 threads) and a workgroup's (256) span on both routes -- W % 8 == 0 is the forward's 16-byte route,
W % 4 == 0 the backward's, every other width the one-float routes; the last output column reads one input column at odd
W and two at even W -- and two shapes past one sweep of the capped grid (STRIDED; tests/test_stem_pool_cases.py proves from
``glue.stem_pool_plan`` which launches stride)."""
import functools

import numpy as np

TABLE_SHAPES = [(1, 1, 1, 1), (1, 1, 1, 2), (1, 1, 2, 1), (1, 1, 2, 2), (1, 2, 3, 3), (2, 3, 5, 7), (1, 2, 4, 4), (2, 1, 6, 8),
                (1, 1, 1, 257), (1, 1, 129, 1), (3, 64, 6, 20)]
WIDTHS = (63, 64, 65, 127, 128, 129, 255, 256, 257)
WIDTH_SHAPES = [(1, 2, H, W) for H in (3, 4) for W in WIDTHS]
# past one sweep of the grid: on the one-float routes (odd W) forward and backward; on the 16-byte routes forward and backward
STRIDED = {"one_float_routes": (1, 2, 1030, 1023), "sixteen_byte_routes": (1, 8, 1032, 1024)}
STRIDED_FILLINGS = ("relu", "integers")  # where ties dominate; the other fillings add nothing a small shape does not show
SHAPES = TABLE_SHAPES + WIDTH_SHAPES

FILLINGS = ("normal", "relu", "zeros", "threes", "integers", "nan_corner", "nan_shared", "nan_last_column", "nan_pair",
            "neg_inf_plane", "pos_inf")
TIE_FILLINGS = ("relu", "zeros", "threes", "integers")


def out_shape(shape):
    B, C, H, W = shape
    return B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1


def cases():
    return [(s, f) for s in SHAPES for f in FILLINGS] + [(s, f) for s in STRIDED.values() for f in STRIDED_FILLINGS]


def case_id(case):
    (B, C, H, W), filling = case
    return "%dx%dx%dx%d-%s" % (B, C, H, W, filling)


def _rng(shape, filling, salt):
    return np.random.default_rng([salt, FILLINGS.index(filling)] + list(shape))


@functools.lru_cache(None)
def make_input(case):
    """y, float32 (read-only: shared between tests)"""
    shape, filling = case
    B, C, H, W = shape
    rng = _rng(shape, filling, 1)
    y = rng.standard_normal(shape).astype(np.float32)
    if filling == "relu":
        y = np.maximum(y, 0)  # about half the values 0: most windows tie at 0
    elif filling == "zeros":
        y[:] = 0
    elif filling == "threes":
        y[:] = 3
    elif filling == "integers":
        y = rng.integers(-2, 3, shape).astype(np.float32)
    elif filling == "nan_corner":
        y[:, :, 0, 0] = np.nan
    elif filling == "nan_shared":  # odd row, odd column: in four windows where the plane has them
        y[:, :, min(1, H - 1), min(1, W - 1)] = np.nan
    elif filling == "nan_last_column":
        y[:, :, H // 2, W - 1] = np.nan
    elif filling == "nan_pair":  # both in window (0, 0); the later one must win it
        y[:, :, 0, 0] = np.nan
        y[:, :, min(1, H - 1), min(1, W - 1)] = np.nan
    elif filling == "neg_inf_plane":
        y[0, 0] = -np.inf
    elif filling == "pos_inf":
        y[B - 1, C - 1, H // 2, W // 2] = np.inf
    y.setflags(write=False)
    return y


@functools.lru_cache(None)
def make_cotangents(case, integer):
    """(g_p, g_y), float32 and read-only; ``integer``: values in -8 .. 8, whose sums of five are exact in any order"""
    shape, filling = case
    rng = _rng(shape, filling, 2 + int(integer))
    out = []
    for s in (out_shape(shape), shape):
        g = rng.integers(-8, 9, s).astype(np.float32) if integer else rng.standard_normal(s).astype(np.float32)
        g.setflags(write=False)
        out.append(g)
    return tuple(out)


def plan(shape, aligned=True):
    """(OH, OW, workgroups forward, workgroups backward, per thread forward, per thread backward), from the library"""
    from mal_amd.glue import stem_pool_plan
    return stem_pool_plan(*shape, aligned)


def sweeps(shape, aligned=True, threads=256):
    """(forward, backward): how many times the launch's grid passes over its units"""
    B, C, H, W = shape
    OH, OW, bf, bb, vf, vb = plan(shape, aligned)
    uf, ub = B * C * OH * (OW // vf), B * C * H * (W // vb)
    return -(-uf // (bf * threads)), -(-ub // (bb * threads))
