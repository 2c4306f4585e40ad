"""The Adam update of mal_amd/csrc/mal_adam.hip (mal_amd.optim.FlatAdam) restated from its definition alone, in plain fp32
torch CPU operators: every operator below is ONE correctly rounded fp32 operation (tensor op tensor, or tensor op Python
scalar, which torch casts to fp32 exactly as the kernel's arguments are cast), none of them fused.  The one exception is
the square root: ``torch.sqrt`` of a large fp32 CPU tensor goes through a vector maths library whose result is off by one ulp
in about 0.7 % of the elements (numpy's and the GPU's are correctly rounded), so it is taken in fp64 and rounded to fp32 --
which is the correctly rounded fp32 square root, 53 bits being more than 2 x 24 + 2.

    m' = m + (g - m) * c1            c1 = 1 - beta1
    v' = v * beta2 + (c2 * g) * g    c2 = 1 - beta2
    den = sqrt(v') / bs + eps        bs = sqrt(1 - beta2^t)
    p' = p + a * (m' / den)          a  = -lr / (1 - beta1^t)

the scalars formed in double as ``torch.optim.Adam`` forms them.  ``step64`` evaluates the same recurrence in fp64 (scalars
unrounded): the yardstick both this restatement and ``torch.optim.Adam`` are measured against
(tests/test_flat_adam_cases.py), since torch's own CPU kernels fuse multiply-adds in their vectorised bodies and not in
their scalar tails and so do not agree with themselves bit for bit across tensor sizes."""
import torch


def scalars(lr, betas, eps, t):
    """(c1, beta2, c2, bs, eps, a) of step t >= 1 as Python doubles"""
    beta1, beta2 = betas
    step = float(t)
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return 1 - beta1, beta2, 1 - beta2, bias_correction2 ** 0.5, eps, -(lr / bias_correction1)


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def step32(p, g, m, v, t, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """one update of fp32 CPU tensors -> (p', m', v'); the inputs are not modified"""
    assert all(x.dtype == torch.float32 and x.device.type == "cpu" for x in (p, g, m, v))
    c1, b2, c2, bs, e, a = (_f32(x) for x in scalars(lr, betas, eps, t))  # rounded once, as the kernel's arguments
    m = m + (g - m) * c1
    v = v * b2 + (g * c2) * g
    den = torch.sqrt(v.double()).float() / bs + e  # the correctly rounded fp32 square root (module docstring)
    p = p + (m / den) * a
    return p, m, v


def step64(p, g, m, v, t, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """the same recurrence in fp64 with unrounded scalars; ``g`` may be fp32 (it is the data), the state is fp64"""
    c1, b2, c2, bs, e, a = scalars(lr, betas, eps, t)
    g = g.double()
    m = m + (g - m) * c1
    v = v * b2 + (g * c2) * g
    den = torch.sqrt(v) / bs + e
    p = p + (m / den) * a
    return p, m, v


def run32(p0, grads, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, m0=None, v0=None, t0=0):
    """len(grads) steps from (p0, m0, v0) at step number t0 -> (p, m, v); ``lr`` a number or one per step"""
    p, m, v = p0.clone(), (torch.zeros_like(p0) if m0 is None else m0.clone()), (torch.zeros_like(p0) if v0 is None else v0.clone())
    for k, g in enumerate(grads):
        p, m, v = step32(p, g, m, v, t0 + k + 1, lr[k] if isinstance(lr, (list, tuple)) else lr, betas, eps)
    return p, m, v


def run64(p0, grads, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    p, m, v = p0.double(), torch.zeros_like(p0, dtype=torch.float64), torch.zeros_like(p0, dtype=torch.float64)
    for k, g in enumerate(grads):
        p, m, v = step64(p, g, m, v, k + 1, lr, betas, eps)
    return p, m, v


def rel_l2(x, ref):
    """L2-relative distance of x from the fp64 reference"""
    ref = ref.double()
    return float((x.double() - ref).norm() / ref.norm())
