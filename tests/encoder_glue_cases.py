"""The case table of the encoder glue (mal_amd.glue.bn_join, mal_amd/csrc/mal_bn.hip) and an fp64 restatement of what it
computes, forward and backward, from the formulas alone.  Shared by tests/test_encoder_glue_cases.py (CPU) and
tests/test_gpu_encoder_glue.py (GPU); the reference for every number is PyTorch itself.

    training:  mean = sum(x)/N, var = sum((x-mean)^2)/N, invstd = 1/sqrt(var + eps), xh = (x-mean)*invstd
               pre = gamma*xh + beta (+ r),  y = relu ? max(pre, 0) : pre
               running_mean <- (1-m)*running_mean + m*mean,  running_var <- (1-m)*running_var + m*var*N/(N-1)
    backward:  g' = relu ? g*[y > 0] : g,  dbeta = sum g',  dgamma = sum g'*xh,
               dx = gamma*invstd*(g' - dbeta/N - xh*dgamma/N),  dr = g'
"""
import functools

import torch

EPS = 1e-5
MODES = ("relu", "residual_relu", "plain")  # stem bn1 and each block's bn1; each block's bn2; the downsample norms
MEANS = (0.0, 100.0)                         # input mean at std 1; mean 100 goes with momentum 0.01 in the first position
MOMENTA = (0.1, 0.01)
# (B,C,H,W).  The last one is this file's: H*W odd (the 4-byte path) with more than one block per channel.
TABLE_SHAPES = [(2, 3, 1, 1), (1, 1, 1, 2), (2, 5, 3, 7), (4, 7, 9, 33), (3, 64, 6, 20), (2, 512, 3, 5), (2, 64, 48, 160),
                (2, 64, 96, 320), (5, 3, 27, 33)]
SCAN = (2, 4, 4)   # C, H, W of the scan over B that finds the boundaries of the plan
SCAN_B = 8192      # N = B*16 up to 131072: past the stem's elements per channel at B=12 divided by its 32 blocks


@functools.lru_cache(None)
def plan(B, C, H, W):
    from mal_amd.glue import bn_join_plan
    return bn_join_plan(B, C, H, W)


@functools.lru_cache(None)
def boundary_shapes():
    """a shape on each side of every change of blocks-per-channel along B at SCAN's (C,H,W), read from the library"""
    C, H, W = SCAN
    out, prev = [], plan(1, C, H, W)[0]
    for B in range(2, SCAN_B + 1):
        cur = plan(B, C, H, W)[0]
        if cur != prev:
            out += [(B - 1, C, H, W), (B, C, H, W)]
        prev = cur
    return out


def shapes():
    return TABLE_SHAPES + boundary_shapes()


def cases():
    """(shape, mode, mean)"""
    return [(s, m, mu) for s in shapes() for m in MODES for mu in MEANS]


def case_id(case):
    (B, C, H, W), mode, mean = case
    return "%dx%dx%dx%d-%s-mean%d" % (B, C, H, W, mode, int(mean))


def special_channels(C):
    """(index with gamma = 0, index with gamma < 0, constant channel), None where C has no room"""
    return (0 if C >= 2 else None, 1 if C >= 2 else None, 2 if C >= 3 else (0 if C == 2 else None))


def make_inputs(case, seed=0):
    """fp32 CPU tensors: x, r (None without a residual), g, gamma, beta, running_mean, running_var"""
    (B, C, H, W), mode, mean = case
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64) + mean
    zero, neg, const = special_channels(C)
    if const is not None:
        x[:, const] = mean + 0.75
    x = x.float()
    r = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64).float() if mode == "residual_relu" else None
    g = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64).float()
    gamma = torch.randn(C, generator=gen, dtype=torch.float64)
    if zero is not None:
        gamma[zero] = 0.0
    if neg is not None:
        gamma[neg] = -gamma[neg].abs() - 0.5
    beta = 0.5 * torch.randn(C, generator=gen, dtype=torch.float64)
    rm = 0.1 * torch.randn(C, generator=gen, dtype=torch.float64) + mean
    rv = 0.5 + torch.rand(C, generator=gen, dtype=torch.float64)
    return x, r, g, gamma.float(), beta.float(), rm.float(), rv.float()


def relu_of(mode):
    return mode != "plain"


# ------------------------------------------------------------------------------------------------ the restatement, fp64
def statistics(x):
    """-> (mean, biased var) per channel, two passes"""
    N = x.shape[0] * x.shape[2] * x.shape[3]
    mean = x.sum((0, 2, 3)) / N
    var = ((x - mean.view(1, -1, 1, 1)) ** 2).sum((0, 2, 3)) / N
    return mean, var


def forward(x, r, gamma, beta, relu, mean, var, eps=EPS):
    """-> (y, pre, xh); (mean, var) are the batch's in training mode, the running ones in eval mode"""
    v = lambda t: t.view(1, -1, 1, 1)
    xh = (x - v(mean)) * v(1.0 / torch.sqrt(var + eps))
    pre = v(gamma) * xh + v(beta)
    if r is not None:
        pre = pre + r
    return (torch.clamp(pre, min=0) if relu else pre), pre, xh


def running(rm, rv, mean, var, N, momentum):
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * var * N / (N - 1)


def backward(g, x, gamma, relu, mean, var, mask=None, eps=EPS):
    """-> (dx, dr, dgamma, dbeta).  ``mask`` (bool, y > 0) is required with ``relu``: the caller says whose decisions count."""
    v = lambda t: t.view(1, -1, 1, 1)
    N = x.shape[0] * x.shape[2] * x.shape[3]
    invstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - v(mean)) * v(invstd)
    gp = g * mask.to(g.dtype) if relu else g
    dbeta = gp.sum((0, 2, 3))
    dgamma = (gp * xh).sum((0, 2, 3))
    dx = v(gamma * invstd) * (gp - v(dbeta) / N - xh * v(dgamma) / N)
    return dx, gp, dgamma, dbeta


def l2rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))
