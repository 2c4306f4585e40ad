"""A numpy restatement of the stem max-pool (mal_amd.glue.stem_pool, mal_amd/csrc/mal_pool.hip) from its definition alone:

    p = F.max_pool2d(y, kernel_size=3, stride=2, padding=1)          y (B,C,H,W), any floating dtype

Window (oh, ow) covers rows 2oh-1 .. 2oh+1 and columns 2ow-1 .. 2ow+1 clipped to the plane.  The winner: start from -inf and
the window's first element; scan the clipped window row-major; a value replaces the running maximum when
``val > max or isnan(val)``.  tests/test_stem_pool_cases.py holds this to torch on the CPU (values, indices, gradient routing);
torch is the arbiter.  ``ge=True`` turns the comparison to ``>=`` (the LAST of equal maxima): the wrong rule, kept so that the
test can show its tie fillings tell the two apart."""
import numpy as np


def out_size(n):
    return (n - 1) // 2 + 1


def forward(y, ge=False):
    """-> (p, code, index): the pooled values, the winner's position kh*3 + kw in the unclipped window (uint8) and its flat
    index h*W + w in the plane (int64, what torch returns with return_indices=True)"""
    y = np.asarray(y)
    B, C, H, W = y.shape
    OH, OW = out_size(H), out_size(W)
    oh, ow = np.arange(OH), np.arange(OW)
    m = np.full((B, C, OH, OW), -np.inf, dtype=y.dtype)
    code = np.broadcast_to(((oh == 0) * 3)[:, None] + (ow == 0)[None, :], (B, C, OH, OW)).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        for kh in range(3):
            h = 2 * oh + kh - 1
            vh = (h >= 0) & (h < H)
            for kw in range(3):
                w = 2 * ow + kw - 1
                vw = (w >= 0) & (w < W)
                v = y[:, :, np.clip(h, 0, H - 1)[:, None], np.clip(w, 0, W - 1)[None, :]]
                take = (vh[:, None] & vw[None, :]) & (((v >= m) if ge else (v > m)) | np.isnan(v))
                m = np.where(take, v, m)
                code = np.where(take, np.uint8(kh * 3 + kw), code)
    return m, code, index_of(code, H, W)


def index_of(code, H, W):
    """codes (B,C,OH,OW) -> flat indices h*W + w of the winners (int64)"""
    code = np.asarray(code).astype(np.int64)
    OH, OW = code.shape[2:]
    h = 2 * np.arange(OH)[:, None] + code // 3 - 1
    w = 2 * np.arange(OW)[None, :] + code % 3 - 1
    assert (h >= 0).all() and (h < H).all() and (w >= 0).all() and (w < W).all(), "a code points outside the plane"
    return h * W + w


def backward(g_p, g_y, code, shape, dtype=np.float64):
    """-> dy = g_y (0 without) + every g_p routed to its window's winner, summed in ``dtype``"""
    B, C, H, W = shape
    OH, OW = out_size(H), out_size(W)
    g_p = np.asarray(g_p).astype(dtype)
    index_of(code, H, W)  # every code inside the plane
    pad = np.zeros((B, C, 2 * OH + 1, 2 * OW + 1), dtype=dtype)  # row h + 1, column w + 1
    for k in range(9):
        kh, kw = divmod(k, 3)
        pad[:, :, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] += np.where(code == k, g_p, 0)  # one k: distinct targets
    dy = pad[:, :, 1:H + 1, 1:W + 1]
    return dy if g_y is None else dy + np.asarray(g_y).astype(dtype)
