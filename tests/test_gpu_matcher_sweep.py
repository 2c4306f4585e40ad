"""GPU: mal_amd.matcher.HungarianMatcher over the case table of tests/matcher_checks.py (sizes around 64 and at 128 on both
sides, tail words, a second pack trip, mixed mask kinds, wide classes, a zero weight); the gates are stated there."""
import numpy as np
import pytest
import torch

from tests import matcher_checks as K
from tests import matcher_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


class _Inst:
    def __init__(self, classes, masks):
        self.pred_classes, self.pred_masks = classes, masks

    def __len__(self):
        return len(self.pred_classes)


def as_kind(d, s, kind):
    m = torch.from_numpy(d["masks_" + s])
    if kind == "bool":
        return m.to(DEV)
    if kind == "uint8":  # non-zero = set, whatever the byte
        return (m.to(torch.uint8) * torch.from_numpy(d["bytes_" + s])).to(DEV)
    return m.float().to(DEV)


def run(d, kinds):
    from mal_amd.matcher import HungarianMatcher
    w_class, w_mask, w_dice = d["weights"]
    m = HungarianMatcher(cost_class=w_class, cost_mask=w_mask, cost_dice=w_dice)
    sets = [_Inst(torch.from_numpy(d["class_" + s]).to(DEV), as_kind(d, s, kind)) for s, kind in zip(("n", "m", "0"), kinds)]
    sn, sm = m(*sets)
    assert sn.is_cuda and sm.is_cuda and sn.dtype == torch.int64 and sm.dtype == torch.int64
    assert sn.is_contiguous() and sm.is_contiguous()
    C1, C2 = m.last_costs
    assert C1.dtype == torch.float32 and C2.dtype == torch.float32
    return sn.cpu().numpy(), sm.cpu().numpy(), C1.cpu().numpy(), C2.cpu().numpy()


@pytest.mark.parametrize("name", list(K.CASES))
def test_case(name):
    d = K.make(name)
    D1, D2 = K.reference(name)
    n_n, n_m, n_0 = d["sizes"]
    sn, sm, C1, C2 = out = run(d, d["kinds"])
    # gate 1
    assert len(sn) == len(sm) <= min(d["sizes"])
    assert len(set(sn.tolist())) == len(sn) and len(set(sm.tolist())) == len(sm)
    assert all(0 <= v < n_n for v in sn.tolist()) and all(0 <= v < n_m for v in sm.tolist())
    assert C1.shape == (n_n, n_0) and C2.shape == (n_m, n_0)
    # gate 2
    for C, Dm in ((C1, D1), (C2, D2)):
        if Dm.size:
            excess = np.abs(C.astype(np.float64) - Dm) - K.cost_bound(Dm)
            print("%s: max |C - fp64| = %.3g, worst excess over the bound %.3g" % (name, np.abs(C - Dm).max(), excess.max()))
            assert float(excess.max()) <= 0.0
    # gate 3: the stated algorithm on the kernel's own matrices, ties included
    want, _ = R.match(C1, C2) if min(d["sizes"]) else (np.zeros((0, 2), np.int64), None)
    got = np.stack([sn, sm], 1).reshape(-1, 2)
    assert np.array_equal(got, want), (got[:8].tolist(), want[:8].tolist())
    # gate 4
    if d["unique"]:
        assert np.array_equal(got, R.match(D1, D2)[0])
    # gate 5: across mask kinds, across two runs
    for kinds in (("bool",) * 3, d["kinds"][1:] + d["kinds"][:1], d["kinds"]):
        for mine, other in zip(out, run(d, kinds)):
            assert mine.tobytes() == other.tobytes(), kinds
