"""CPU: ``mal_cost_volume`` refuses bad arguments before any device work (mal_amd/csrc/mal_costvol.hip returns ahead of its
first launch), and the wrapper refuses lookup features that do not match the current ones.  Follows
tests/test_step_scales.py::test_warp_scales_rejects_bad_arguments_without_a_device."""
import pytest
import torch

EINVAL, ESHAPE = -1, -2
FAKE = 0x1000  # a non-null pointer that is never dereferenced: every call below fails before any device work


@pytest.fixture(scope="module")
def lib():
    from mal_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def call(lib, B=2, F=2, C=64, D=8, h=16, w=28, null=()):
    """mal_cost_volume with fake pointers; ``null``: names of pointer arguments passed as NULL"""
    names = ("current_feats", "lookup_feats", "poses", "K", "inv_K", "depth_bins")
    ins = [None if n in null else FAKE for n in names]
    outs = [None if n in null else FAKE for n in ("cost_volume", "missing_mask", "masked_cost_volume", "lowest_cost", "confidence_mask")]
    return lib.mal_cost_volume(*ins, B, F, C, D, h, w, 1e-7, 1, *outs, None)


@pytest.mark.parametrize("bad", [dict(C=63), dict(C=65), dict(D=0), dict(D=257), dict(h=4), dict(w=4), dict(B=0), dict(F=0),
                                 dict(B=-1), dict(F=-2), dict(D=-3)], ids=lambda d: "%s=%d" % next(iter(d.items())))
def test_cost_volume_rejects_bad_shapes_without_a_device(lib, bad):
    assert call(lib, **bad) == ESHAPE


def test_cost_volume_rejects_sizes_past_the_element_bound_without_a_device(lib):
    """2e9 / 4 elements, on the volume (B*D*h*w) and on the lookup features (B*F*h*w*C).  A size just under the bound gets
    past the shape checks: with a null required pointer it is MAL_EINVAL, not MAL_ESHAPE"""
    assert 8 * 256 * 512 * 512 > 2.0e9 / 4 > 7 * 256 * 512 * 512
    assert call(lib, B=8, F=1, D=256, h=512, w=512) == ESHAPE
    assert call(lib, B=7, F=1, D=256, h=512, w=512, null=("current_feats",)) == EINVAL
    assert 4 * 8 * 512 * 512 * 64 > 2.0e9 / 4 > 4 * 7 * 512 * 512 * 64
    assert call(lib, B=4, F=8, D=1, h=512, w=512) == ESHAPE
    assert call(lib, B=4, F=7, D=1, h=512, w=512, null=("current_feats",)) == EINVAL


@pytest.mark.parametrize("name", ["current_feats", "lookup_feats", "poses", "K", "inv_K", "depth_bins", "cost_volume"])
def test_cost_volume_rejects_a_null_required_pointer_without_a_device(lib, name):
    assert call(lib, null=(name,)) == EINVAL


def test_shape_checks_come_first(lib):
    assert call(lib, C=63, null=("current_feats",)) == ESHAPE


@pytest.mark.parametrize("shape", [(2, 64, 16, 28), (2, 2, 64, 16), (3, 2, 64, 16, 28), (2, 2, 32, 16, 28), (2, 2, 64, 16, 27),
                                   (2, 2, 64, 15, 28)], ids=lambda s: "x".join(map(str, s)))
def test_wrapper_rejects_lookup_feats_that_do_not_match(shape):
    """wrong rank, batch, channel count or size: refused by shape, before the wrapper looks at devices or the library"""
    from mal_amd import costvol
    from mal_amd._lib import MalError
    eye = torch.eye(4).expand(2, 4, 4)
    for fn in (costvol.match_features, costvol.cost_volume_outputs):
        with pytest.raises(MalError, match="lookup_feats must be"):
            fn(torch.zeros(2, 64, 16, 28), torch.zeros(*shape), torch.zeros(2, 2, 4, 4), eye, eye, torch.linspace(0.5, 20.0, 8))
