"""CPU: the restatement of the decoder glue (tests/decoder_glue_restated.py) against torch's own composition and autograd in
fp64 at the shared case table; the term count; the argument checks of mal_decoder_join_* (no device is touched); and the
two properties of DepthDecoder(fused_glue=True) that need no device: CPU tensors raise, the state dict is unchanged."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import decoder_glue_restated as R

IDS = [R.case_id(c) for c in R.CASES]


def torch_composition(x, skip, up, elu):
    y = F.elu(x) if elu else x
    if up == 2:
        y = F.interpolate(y, scale_factor=2, mode="nearest")
    if skip is not None:
        y = torch.cat([y, skip], 1)
    return F.pad(y, (1, 1, 1, 1), mode="reflect")


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_restatement_matches_torch_fp64(case):
    up, elu, B, C, Cs, h, w = case
    x, skip, g = (None if a is None else a.astype(np.float64) for a in R.make_inputs(case))
    tx = torch.from_numpy(x).requires_grad_(True)
    ts = torch.from_numpy(skip).requires_grad_(True) if skip is not None else None
    out = torch_composition(tx, ts, up, elu)
    assert tuple(out.shape) == (B, C + Cs, up * h + 2, up * w + 2)
    mine = R.forward(x, skip, up, elu)
    assert np.abs(mine - out.detach().numpy()).max() <= 1e-12
    out.backward(torch.from_numpy(g))
    gx, gskip = R.backward(g, x, up, elu)
    scale = max(1.0, float(np.abs(tx.grad.numpy()).max()))
    assert np.abs(gx - tx.grad.numpy()).max() <= 1e-12 * scale
    if skip is not None:
        assert np.abs(gskip - ts.grad.numpy()).max() <= 1e-12
    else:
        assert gskip.shape[1] == 0


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_term_count(case):
    up, elu, B, C, Cs, h, w = case
    nx, ns = R.term_counts(h, w, up)
    assert nx.min() >= 1 and ns.min() >= 1
    assert nx.max() <= 16 and ns.max() <= 9
    assert (nx.max() == 16) == (up == 2 and h == 1 and w == 1)
    if h > 1 and w > 1:  # 12 when exactly one of h, w is 1 under up = 2: both rows of the block are reflected into
        assert nx.max() <= 9
    elif up == 2 and (h, w) != (1, 1):
        assert nx.max() == 12
    # every cotangent element is received exactly once
    assert nx.sum() == (up * h + 2) * (up * w + 2) == ns.sum()


@pytest.fixture(scope="module")
def lib():
    from mal_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_invalid_arguments_are_refused_without_a_device(lib):
    p, n, E = 4096, None, -1  # a non-null "pointer" that is never dereferenced: every call below returns before any HIP call
    fwd, bwd = lib.mal_decoder_join_fwd, lib.mal_decoder_join_bwd
    ok = dict(B=2, C=3, Cs=2, h=4, w=5, up=2, elu=1)

    def f(x=p, skip=p, out=p, **kw):
        a = dict(ok, **kw)
        return fwd(x, skip, out, a["B"], a["C"], a["Cs"], a["h"], a["w"], a["up"], a["elu"], n)

    def b(g=p, x=p, gx=p, gskip=p, **kw):
        a = dict(ok, **kw)
        return bwd(g, x, gx, gskip, a["B"], a["C"], a["Cs"], a["h"], a["w"], a["up"], a["elu"], n)

    assert f(x=n) == E and f(out=n) == E and f(skip=n) == E
    assert b(g=n) == E and b(x=n) == E
    for call in (f, b):
        for bad in (dict(up=0), dict(up=3), dict(up=4), dict(elu=2), dict(elu=-1), dict(B=0), dict(C=0), dict(h=0), dict(w=0),
                    dict(B=-1), dict(Cs=-1), dict(up=1, h=1), dict(up=1, w=1),
                    dict(B=64, C=512, h=256, w=256),          # 2^31 + elements
                    dict(B=1, C=1, Cs=0, h=2 ** 30, w=2 ** 30), dict(B=2 ** 31 - 1, C=2 ** 31 - 1)):
            assert call(**bad) == E, (call.__name__, bad)
    # nothing to compute: fine, and still no device call
    assert b(gx=n, gskip=n) == 0
    assert b(gx=n, gskip=p, Cs=0, x=n, elu=0) == 0


def test_fused_decoder_refuses_cpu_tensors(lib):
    from mal_amd import _lib, networks
    dec = networks.DepthDecoder([64, 64, 128, 256, 512], [0], fused_glue=True)
    feats = [torch.rand(1, c, 32 >> i, 48 >> i) for i, c in enumerate([64, 64, 128, 256, 512])]
    with pytest.raises(_lib.MalError):
        dec(feats)
    from mal_amd.glue import decoder_join
    with pytest.raises(_lib.MalError):
        decoder_join(torch.rand(1, 2, 3, 4))
    with pytest.raises(_lib.MalError):
        decoder_join(torch.rand(1, 2, 3, 4), up=3)


def test_fused_decoder_keeps_the_state_dict():
    from mal_amd import harness, networks
    a = networks.DepthDecoder([64, 64, 128, 256, 512], [0])
    b = networks.DepthDecoder([64, 64, 128, 256, 512], [0], fused_glue=True)
    assert a.fused_glue is False and b.fused_glue is True
    ka, kb = list(a.state_dict()), list(b.state_dict())
    assert ka == kb and len(ka) == 22
    assert [(k, tuple(v.shape)) for k, v in a.state_dict().items()] == [(k, tuple(v.shape)) for k, v in b.state_dict().items()]
    assert harness.default_options().fused_decoder is False
    assert harness.default_options(fused_decoder=True).fused_decoder is True
