"""The checker of mal_amd.msda: the arithmetic of the HIP kernel (mal_amd/csrc/mal_msda.hip), which is that of upstream's
``ms_deformable_im2col_gpu_kernel``, restated in numpy in a chosen dtype, plus the module's softmax, location step and four
linear layers (``ops/modules/ms_deform_attn.py:98-124``).  In fp64 it reproduces the reference's fp64 outputs stored in
tests/golden/msda_*.npz (scripts/gen_golden_msda.py) to rounding; in fp32 it is one more fp32 evaluation of the same
function.  Also here: the fixture cases, their loader and the seeded inputs of the GPU sweep."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOOR, MARGIN = 1e-6, 1.25  # the gate: distance <= max(MARGIN x the reference's own fp32 distance, FLOOR)

# tag -> N, M, D, P, levels, Lq (None: Lq = S, self-attention)
CASES = {
    "a": (2, 8, 32, 4, ((6, 20), (3, 10), (2, 5)), None),
    "b": (1, 2, 8, 2, ((5, 7),), 9),
    "c": (2, 4, 6, 3, ((7, 9), (4, 5), (2, 3), (1, 2)), 33),
    "d": (3, 1, 64, 1, ((3, 4),), 5),
    "x": (2, 8, 32, 4, ((8, 16), (4, 8), (2, 4)), None),
}
MODULE_CASES = {"m2": 2, "m4": 4}  # tag -> last dimension of the reference points
MODULE_CFG = dict(d_model=64, n_levels=3, n_heads=4, n_points=2)
MODULE_LEVELS, MODULE_N, MODULE_LQ = ((4, 6), (2, 3), (1, 2)), 2, 20
VALUE_UNIT, LOC_UNIT, WEIGHT_UNIT = 16.0, 4096.0, 4096.0  # the fixtures' inputs are stored as integers in these units
STATE_KEYS = tuple("%s.%s" % (m, p) for m in ("sampling_offsets", "attention_weights", "value_proj", "output_proj")
                   for p in ("weight", "bias"))


def starts_of(levels):
    at, out = 0, []
    for h, w in levels:
        out.append(at)
        at += h * w
    return out, at


def rel_dist(a, b):
    """|| a - b ||_2 / || b ||_2 in fp64; 0 for a == b (an all-zero b included: every sample outside the map), inf for
    any difference from an all-zero b"""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    diff, norm = float(np.linalg.norm(a - b)), float(np.linalg.norm(b))
    if diff == 0.0:
        return 0.0
    return diff / norm if norm > 0.0 else float("inf")


def gate(ref_dist):
    return max(MARGIN * float(ref_dist), FLOOR)


def level_ok(h, w, start, S):
    return 1 <= h <= min(S, 1 << 24) and 1 <= w <= min(S, 1 << 24) and 0 <= start and start + h * w <= S


def core(value, shapes, start, loc, weights, dtype=np.float64):
    """value (N,S,M,D), shapes L x (H,W), start (L), loc (N,Lq,M,L,P,2) in (x, y) order, weights (N,Lq,M,L,P) ->
    (N, Lq, M*D).  Per sample, in this order (the kernel's): x*W - 0.5, y*H - 0.5; the range test y > -1, x > -1, y < H,
    x < W (NaN fails); floor; the four corner weights hh*hw, hh*lw, lh*hw, lh*lw; ((w1 v1 + w2 v2) + w3 v3) + w4 v4 with a
    corner outside the map read as zero; times the attention weight; added to the running sum over p, then l."""
    f = np.dtype(dtype).type
    value, loc, weights = (np.asarray(t, dtype) for t in (value, loc, weights))
    N, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    out = np.zeros((N, Lq, M, D), dtype)
    nn, mm = np.arange(N)[:, None, None], np.arange(M)[None, None, :]
    for l in range(L):
        H, W, st = int(shapes[l][0]), int(shapes[l][1]), int(start[l])
        if not level_ok(H, W, st, S):
            continue
        v = value[:, st:st + H * W].reshape(N, H, W, M, D)

        def corner(iy, ix):
            ok = (iy >= 0) & (iy <= H - 1) & (ix >= 0) & (ix <= W - 1)
            return np.where(ok[..., None], v[nn, np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1), mm], f(0))

        for p in range(P):
            with np.errstate(invalid="ignore", over="ignore"):
                x = loc[:, :, :, l, p, 0] * f(W) - f(0.5)
                y = loc[:, :, :, l, p, 1] * f(H) - f(0.5)
                inside = (y > -1) & (x > -1) & (y < H) & (x < W)
            x, y = np.where(inside, x, f(0)), np.where(inside, y, f(0))
            yl, xl = np.floor(y), np.floor(x)
            lh, lw = y - yl, x - xl
            hh, hw = f(1) - lh, f(1) - lw
            iy, ix = yl.astype(np.int64), xl.astype(np.int64)
            val = (((hh * hw)[..., None] * corner(iy, ix) + (hh * lw)[..., None] * corner(iy, ix + 1))
                   + (lh * hw)[..., None] * corner(iy + 1, ix)) + (lh * lw)[..., None] * corner(iy + 1, ix + 1)
            out += np.where(inside[..., None], weights[:, :, :, l, p, None] * val, f(0))
    assert out.dtype == np.dtype(dtype)
    return out.reshape(N, Lq, M * D)


def softmax(logits, dtype=np.float64):
    """over the last axis, max-subtracted, the sum taken in index order"""
    x = np.asarray(logits, dtype)
    e = np.exp(x - x.max(-1, keepdims=True))
    s = np.zeros(x.shape[:-1], dtype)
    for k in range(x.shape[-1]):
        s = s + e[..., k]
    return e / s[..., None]


def locations(offsets, ref, shapes, dtype=np.float64):
    """offsets (N,Lq,M,L,P,2), ref (N,Lq,L,2|4) -> (N,Lq,M,L,P,2): ops/modules/ms_deform_attn.py:106-112"""
    f = np.dtype(dtype).type
    off, ref = np.asarray(offsets, dtype), np.asarray(ref, dtype)
    P = off.shape[4]
    if ref.shape[-1] == 2:
        wh = np.array([[w, h] for h, w in shapes], dtype)
        return ref[:, :, None, :, None, :] + off / wh[None, None, None, :, None, :]
    return ref[:, :, None, :, None, :2] + off / f(P) * ref[:, :, None, :, None, 2:] * f(0.5)


def module_forward(sd, query, ref, inp, shapes, start, mask=None, dtype=np.float64, n_heads=MODULE_CFG["n_heads"],
                   n_points=MODULE_CFG["n_points"]):
    """the whole module from its state dict ``sd`` -> (output, offsets, logits)"""
    lin = lambda x, name: np.asarray(x, dtype) @ np.asarray(sd[name + ".weight"], dtype).T + np.asarray(sd[name + ".bias"], dtype)
    N, Lq, C = query.shape
    S, L = inp.shape[1], len(shapes)
    value = lin(inp, "value_proj")
    if mask is not None:
        value = np.where(np.asarray(mask, bool)[..., None], np.dtype(dtype).type(0), value)
    value = value.reshape(N, S, n_heads, C // n_heads)
    offsets = lin(query, "sampling_offsets").reshape(N, Lq, n_heads, L, n_points, 2)
    logits = lin(query, "attention_weights").reshape(N, Lq, n_heads, L * n_points)
    w = softmax(logits, dtype).reshape(N, Lq, n_heads, L, n_points)
    out = core(value, shapes, start, locations(offsets, ref, shapes, dtype), w, dtype)
    return lin(out, "output_proj"), offsets, logits


def load_case(tag):
    """a fixture as a dict of numpy arrays: the operator cases hold value, loc, weights (fp32, decoded from the stored
    integers), shapes, start, ref32, ref64, ref_dist; the module cases hold the state dict ``sd``, query, ref, inp, mask (or
    None), shapes, start, out32, out64, ref_dist, offsets, logits, state_keys, state_shapes"""
    z = np.load(os.path.join(GOLDEN, "msda_%s.npz" % tag))
    d = {k: z[k] for k in z.files}
    d["shapes"] = [tuple(int(v) for v in r) for r in d["shapes"]]
    d["start"] = [int(v) for v in d["start"]]
    d["ref_dist"] = float(d["ref_dist"])
    if tag in MODULE_CASES:
        d["sd"] = {k: d.pop("sd." + k) for k in STATE_KEYS}
        d["mask"] = d["mask"] if d["mask"].size else None
        d["state_keys"] = [str(k) for k in d["state_keys"]]
        return d
    d["value"] = d.pop("value_q").astype(np.float32) / np.float32(VALUE_UNIT)
    if "loc_q" in d:  # (case b holds fp32 locations: its boundary samples are not on the grid)
        d["loc"] = d.pop("loc_q").astype(np.float32) / np.float32(LOC_UNIT)
    d["weights"] = d.pop("weights_q").astype(np.float32) / np.float32(WEIGHT_UNIT)
    # the reference's fp32 output, stored as its distance in fp32 ulps from the rounded fp64 output (small integers)
    near = d["ref64"].astype(np.float32)
    d["ref32"] = (near.view(np.int32) + d.pop("ref32_ulps").astype(np.int32)).view(np.float32)
    return d


SWEEP_LEVELS = {1: ((5, 7),), 3: ((6, 9), (3, 4), (1, 1)), 4: ((7, 9), (4, 5), (2, 3), (1, 1)),
                8: ((7, 9), (4, 5), (2, 3), (1, 1), (1, 6), (5, 1), (3, 3), (2, 2))}  # MAL_MSDA_MAX_L levels, two of them thin


def sweep_inputs(seed, N, Lq, M, D, L, P):
    """seeded inputs of the GPU sweep: locations around random centres with a spread that puts about a fifth outside [0,1]"""
    rng = np.random.default_rng(seed)
    levels = SWEEP_LEVELS[L]
    start, S = starts_of(levels)
    value = rng.standard_normal((N, S, M, D)).astype(np.float32)
    loc = (rng.random((N, Lq, 1, 1, 1, 2)) + 0.2 * rng.standard_normal((N, Lq, M, L, P, 2))).astype(np.float32)
    weights = softmax(rng.standard_normal((N, Lq, M, L * P)), np.float64).reshape(N, Lq, M, L, P).astype(np.float32)
    return value, levels, start, loc, weights
