"""numpy restatement of the decoder glue (mal_amd/csrc/mal_glue.hip, mal_amd.glue.decoder_join), in whatever dtype it is
given -- the tests feed it float64:

  H = up*h, W = up*w, src(p) = 1 if p == 0; H-2 if p == H+1; else p-1   (columns: the same with W)
  forward   out[b,c,p,q] = act(x[b,c, src(p)/up, src(q)/up])           c <  C,  act(v) = v > 0 ? v : expm1(v) with elu
            out[b,c,p,q] = skip[b,c-C, src(p), src(q)]                  c >= C
  backward  R(r) = {r+1} u {0 if r == 1} u {H+1 if r == H-2}
            S[b,c,r,s]   = sum_{p in R(r)} sum_{q in R(s)} g[b,c,p,q]
            gskip[b,k]   = S[b,C+k]
            gx[b,c,i,j]  = a' * sum over the up x up block of S[b,c]      a' = 1 (x > 0) or expm1(x) + 1 = y + 1

CASES is the table the CPU and the GPU tests share: (up, elu, B, C, Cs, h, w)."""
import numpy as np

CASES = [
    (2, 1, 1, 1, 0, 1, 1),     # every reflection lands in one block: 16 terms
    (2, 1, 2, 3, 0, 1, 5),
    (2, 1, 1, 2, 5, 3, 2),
    (2, 1, 1, 2, 1, 2, 1),
    (2, 1, 3, 16, 8, 6, 7),    # W+2 = 16
    (2, 0, 2, 4, 4, 5, 8),     # W+2 = 18: the 16-byte alignment of a row start alternates
    (2, 1, 1, 5, 3, 33, 70),   # rows longer than two waves
    (1, 1, 2, 3, 0, 2, 2),
    (1, 0, 1, 2, 0, 3, 5),     # row 1 is also row H-2
    (1, 1, 1, 4, 2, 7, 9),
    (1, 1, 2, 3, 0, 6, 66),
    (1, 1, 1, 2, 0, 5, 131),   # odd W: every residue of the row start mod 4
]
PLANTED = (0.0, -0.0, -1e-30, -100.0, 88.0)


def case_id(case):
    return "up%d_elu%d_B%d_C%d_Cs%d_%dx%d" % case


def make_inputs(case, seed=0):
    """float32 (x, skip or None, g): x ~ N(0, 3^2) with PLANTED written over its first elements in a fixed scatter, skip and
    g ~ N(0, 1); the generator is seeded by the case and ``seed``"""
    up, elu, B, C, Cs, h, w = case
    rng = np.random.default_rng([seed, up, elu, B, C, Cs, h, w])
    x = (3.0 * rng.standard_normal((B, C, h, w))).astype(np.float32)
    flat = x.reshape(-1)
    for k, v in enumerate(PLANTED[:flat.size]):
        flat[(k * 7919) % flat.size if flat.size >= len(PLANTED) else k] = np.float32(v)
    skip = rng.standard_normal((B, Cs, up * h, up * w)).astype(np.float32) if Cs else None
    g = rng.standard_normal((B, C + Cs, up * h + 2, up * w + 2)).astype(np.float32)
    return x, skip, g


def src_index(n):
    """padded index 0..n+1 -> unpadded index (ReflectionPad2d(1) of an extent n >= 2)"""
    s = np.arange(n + 2) - 1
    s[0], s[n + 1] = 1, n - 2
    return s


def act(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def forward(x, skip, up, elu):
    B, C, h, w = x.shape
    sr, sc = src_index(up * h), src_index(up * w)
    y = act(x) if elu else x
    out = y[:, :, sr // up][:, :, :, sc // up]
    if skip is not None and skip.shape[1]:
        out = np.concatenate([out, skip[:, :, sr][:, :, :, sc]], 1)
    return out


def receivers(n):
    """(n, n+2) 0/1 matrix: row r has ones at R(r)"""
    m = np.zeros((n, n + 2))
    for r in range(n):
        m[r, r + 1] = 1
        if r == 1:
            m[r, 0] = 1
        if r == n - 2:
            m[r, n + 1] = 1
    return m


def gathered(g, C, h, w, up):
    """the sums before the activation's factor: (sum for gx (B,C,h,w), gskip (B,Cs,H,W))"""
    H, W = up * h, up * w
    S = np.einsum("rp,bcpq,sq->bcrs", receivers(H).astype(g.dtype), g, receivers(W).astype(g.dtype))
    B = g.shape[0]
    return S[:, :C].reshape(B, C, h, up, w, up).sum((3, 5)), S[:, C:]


def term_counts(h, w, up):
    """terms each element of (gx, gskip) sums, as (h,w) and (H,W) integer arrays"""
    gx, gs = gathered(np.ones((1, 2, up * h + 2, up * w + 2)), 1, h, w, up)
    return np.rint(gx[0, 0]).astype(int), np.rint(gs[0, 0]).astype(int)


def aprime(x):
    return np.where(x > 0, 1.0, np.expm1(np.minimum(x, 0)) + 1.0)


def backward(g, x, up, elu, a=None):
    """(gx, gskip); ``a`` replaces the activation's factor (the GPU test hands in the fp32 one of the forward's own output)"""
    B, C, h, w = x.shape
    sx, gskip = gathered(g, C, h, w, up)
    if elu:
        sx = (aprime(x) if a is None else a) * sx
    return sx, gskip
