"""CPU: the instance matcher's fixtures, its restated checker, its C ABI and the host side of mal_amd.matcher.

tests/golden/matcher_*.npz were written by scripts/gen_golden_matcher.py from the reference's own
``HungarianMatcher.forward`` (manydepth/matcher.py:89-173); tests/matcher_restated.py is the CPU checker the GPU tests
lean on where no fixture exists, so it is held to the fixtures here."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from tests import matcher_restated as R


@pytest.fixture(scope="module")
def lib():
    from mal_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("tag", R.CASES)
def test_restated_matcher_reproduces_the_reference(tag):
    d = R.load_case(tag)
    C1 = R.costs_fp32(d["masks_n"], d["masks_0"], d["class_n"], d["class_0"])
    C2 = R.costs_fp32(d["masks_m"], d["masks_0"], d["class_m"], d["class_0"])
    assert C1.dtype == np.float32 and C1.shape == d["C1"].shape and C2.shape == d["C2"].shape
    for mine, ref in ((C1, d["C1"]), (C2, d["C2"])):
        if ref.size:
            assert float(np.abs(mine.astype(np.float64) - ref.astype(np.float64)).max()) <= 1e-7
    pairs, targets = R.match(C1, C2)
    assert np.array_equal(pairs, d["pairs"]) and np.array_equal(targets, d["targets"])
    # the fp64 evaluation of the same formula has the same optimum (the fixtures' margins are >= 1e-4)
    D1 = R.costs_fp64(d["masks_n"], d["masks_0"], d["class_n"], d["class_0"])
    D2 = R.costs_fp64(d["masks_m"], d["masks_0"], d["class_m"], d["class_0"])
    assert np.array_equal(R.match(D1, D2)[0], d["pairs"])
    assert float(d["margin"].min()) >= 1e-4


def test_fixture_shapes_are_the_cases_of_the_design():
    want = {"a": (5, 13, 3, 3, 2), "b": (24, 40, 5, 4, 3), "c": (32, 64, 70, 66, 6), "d": (32, 64, 6, 6, 70),
            "e": (192, 640, 20, 20, 8), "f": (24, 40, 4, 0, 3)}
    for tag, shape in want.items():
        d = R.load_case(tag)
        assert (d["H"], d["W"], len(d["masks_n"]), len(d["masks_m"]), len(d["masks_0"])) == shape
        assert len(d["pairs"]) <= min(shape[2:])
    assert len(R.load_case("f")["pairs"]) == 0
    assert len(np.unique(R.load_case("b")["class_n"])) > 1


@pytest.mark.parametrize("shape", [(4, 6), (6, 4), (5, 5), (1, 3), (3, 1)])
def test_restated_solver_is_optimal(shape):
    """against every injection of the smaller side into the larger one"""
    rng = np.random.default_rng(shape[0] * 10 + shape[1])
    for _ in range(5):
        C = rng.random(shape)
        rows, cols = R.linear_sum_assignment(C)
        assert len(rows) == min(shape) and len(set(rows)) == len(rows) and len(set(cols)) == len(cols)
        small, large = min(shape), max(shape)
        T = C if shape[0] <= shape[1] else C.T
        best = min(sum(T[i, p[i]] for i in range(small)) for p in itertools.permutations(range(large), small))
        assert abs(R.assignment_cost(C, rows, cols) - best) <= 1e-12
    ties = np.ones(shape)
    rows, cols = R.linear_sum_assignment(ties)
    assert len(set(rows)) == len(set(cols)) == min(shape)


def test_symbols_are_exported(lib):
    import mal_amd
    from mal_amd import _lib, matcher
    assert mal_amd.HungarianMatcher is matcher.HungarianMatcher and "HungarianMatcher" in mal_amd.__all__
    for name in ("mal_match", "mal_match_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert lib.mal_struct_bytes(7) == ctypes.sizeof(_lib.MatchArgs) > 0
    assert lib.mal_version() == 100
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mal_hip.h")).read()
    assert "#define MAL_MATCH_MAX %d" % _lib.MATCH_MAX in text


def _args(**kw):
    from mal_amd import _lib
    a = _lib.MatchArgs()
    fake = 0x1000  # never dereferenced: every call below is refused before any HIP call
    for n in ("masks_n", "masks_m", "masks_0", "class_n", "class_m", "class_0", "C1", "C2", "slice_n", "slice_m", "result", "ws"):
        setattr(a, n, fake)
    a.n_n, a.n_m, a.n_0, a.H, a.W = 3, 3, 2, 5, 13
    a.cost_class = a.cost_mask = a.cost_dice = 1.0
    a.ws_bytes = 1 << 20
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_validation_without_device(lib):
    call = lambda **kw: lib.mal_match(ctypes.byref(_args(**kw)))
    assert lib.mal_match(None) == -1
    for n in ("n_n", "n_m", "n_0"):
        assert call(**{n: 129}) == -1 and call(**{n: -1}) == -1
    assert call(H=0) == -1 and call(W=0) == -1 and call(H=-4) == -1
    assert call(H=1 << 16, W=1 << 16) == -1
    for n in ("masks_n", "masks_m", "masks_0", "class_n", "class_m", "class_0", "C1", "C2", "slice_n", "slice_m", "result", "ws"):
        assert call(**{n: None}) == -1, n
    assert call(kind_m=2) == -1 and call(kind_0=-1) == -1
    assert call(cost_class=0.0, cost_mask=0.0, cost_dice=0.0) == -1      # matcher.py:86
    assert call(cost_dice=float("nan")) == -1
    assert call(ws_bytes=64) == -3
    need = lib.mal_match_workspace_bytes(3, 3, 2, 5, 13)
    assert need > 0 and call(ws_bytes=need - 1) == -3
    assert lib.mal_match_workspace_bytes(129, 3, 2, 5, 13) == 0 and lib.mal_match_workspace_bytes(3, 3, 2, 0, 13) == 0
    assert lib.mal_match_workspace_bytes(3, 3, -1, 5, 13) == 0
    assert lib.mal_match_workspace_bytes(20, 20, 8, 192, 640) > lib.mal_match_workspace_bytes(20, 20, 8, 96, 320) > need
    # the packed rows and the counts of 128 + 128 + 128 masks must fit
    assert lib.mal_match_workspace_bytes(128, 128, 128, 192, 640) >= 384 * (192 * 640 // 64) * 8 + 384 * 4


class _Inst:
    def __init__(self, classes, masks):
        self.pred_classes, self.pred_masks = classes, masks

    def __len__(self):
        return len(self.pred_classes)


def test_host_side_of_the_matcher(lib):
    from mal_amd import _lib
    from mal_amd.matcher import HungarianMatcher
    with pytest.raises(AssertionError):
        HungarianMatcher(cost_class=0, cost_mask=0, cost_dice=0)
    m = HungarianMatcher(cost_class=2, cost_mask=0, cost_dice=5, ins_threshold=0.3)
    assert repr(m) == "Matcher HungarianMatcher\n    cost_class: 2\n    cost_mask: 0\n    cost_dice: 5"
    assert m.ins_threshold == 0.3 and m.last_costs is None
    inst = _Inst(torch.zeros(2, dtype=torch.int64), torch.zeros(2, 5, 13, dtype=torch.bool))
    with pytest.raises(_lib.MalError):
        m(inst, inst, inst)
    with pytest.raises(_lib.MalError):
        m.memory_efficient_forward(inst, inst, inst)


# ---------------------------------------------------------------- the sweep's case table (tests/matcher_checks.py)
def test_sweep_table_holds_the_sizes_shapes_and_inputs_of_the_design():
    from tests import matcher_checks as K
    specs = list(K.CASES.values())
    assert set(K.REQUIRED_SIZES) <= {c["sizes"] for c in specs}
    assert {k for k in range(3)} == {k for c in specs for k in range(3) if c["sizes"][k] == 0 and sum(c["sizes"]) > 0}
    assert set(K.REQUIRED_SHAPES) <= {(c["H"], c["W"]) for c in specs}
    assert K.nw(96, 96) == 144 > 16 * 8 and K.nw(50, 173) == 136 and (50 * 173) % 64 == 10 and K.nw(5, 13) == 2
    assert {"rand", "proto", "ellipse"} == {c["gen"] for c in specs}
    assert {"equal", "distinct", "high", "mixed"} == {c["classes"] for c in specs}
    assert {(1.0, 1.0, 1.0), (0.0, 1.0, 1.0), (1.0, 1.0, 0.0)} == {c["weights"] for c in specs}
    assert any(len(set(c["kinds"])) == 3 for c in specs) and all(set(c["kinds"]) <= set(K.KINDS) for c in specs)
    big = [c for c in specs if min(c["sizes"]) > 64]
    assert len(big) >= 3  # a lane owns a row and a column in two registers
    d = K.make("rand_128x128x128_96x96_second_pack_trip")
    for s in ("n", "m", "0"):
        counts = d["masks_" + s].reshape(128, -1).sum(1)
        assert counts.min() == 0 and counts.max() == 96 * 96  # an empty and a full mask among the instances
        assert set(np.unique(d["bytes_" + s]).tolist()) == set(K.MASK_BYTES)
    hi = K.make("rand_128x128x128_50x173_dice_weight_zero")
    both = np.concatenate([hi["class_n"], hi["class_0"]])
    assert len(np.unique(both)) > 1 and len(np.unique(both.astype(np.int32))) == 1  # differ above bit 32 only
    D1, _ = K.reference("rand_128x128x128_50x173_dice_weight_zero")
    assert set(np.unique(D1).tolist()) <= {0.0, 1.0}  # the cost is 0 / 1: every path a tie
    dist = K.make("rand_70x100x128_5x13")
    assert len(np.unique(np.concatenate([dist["class_n"], dist["class_m"], dist["class_0"]]))) == 70 + 100 + 128


def _scipy_lsa():
    try:
        from scipy.optimize import linear_sum_assignment
        return linear_sum_assignment
    except Exception:
        return None


@pytest.mark.parametrize("name", __import__("tests.matcher_checks", fromlist=["CASES"]).CASES)
def test_restated_solver_is_certified_on_every_sweep_matrix(name):
    """complementary slackness: u_i + v_j <= C_ij + 1e-12 everywhere, equality on the assigned edges, v <= 0 and v = 0 on
    unassigned columns -- on the fp64 matrices and on their fp32 roundings (what the kernel hands to its solver)"""
    from tests import matcher_checks as K
    lsa = _scipy_lsa()
    for D in K.reference(name):
        for C in (D, D.astype(np.float32).astype(np.float64)):
            rows, cols, u, v = R.linear_sum_assignment(C, return_duals=True)
            assert len(rows) == min(C.shape)
            if C.size == 0:
                continue
            gap = R.certify(C, rows, cols, u, v)
            assert abs(gap) <= 1e-9
            if lsa is not None:
                r2, c2 = lsa(C)
                assert abs(R.assignment_cost(C, rows, cols) - float(C[r2, c2].sum())) <= 1e-9
    if K.CASES[name]["unique"]:
        D1, D2 = K.reference(name)
        for D in (D1, D2):
            F = D.astype(np.float32).astype(np.float64)
            assert R.margin_of(D) >= K.MARGIN and R.margin_of(F) >= K.MARGIN
        assert np.array_equal(R.match(D1, D2)[0], R.match(D1.astype(np.float32), D2.astype(np.float32))[0])


def test_certificate_refuses_a_suboptimal_assignment():
    C = np.array([[1.0, 2.0, 9.0], [2.0, 1.0, 9.0]])
    rows, cols, u, v = R.linear_sum_assignment(C, return_duals=True)
    assert cols.tolist() == [0, 1] and R.certify(C, rows, cols, u, v) == 0.0
    with pytest.raises(AssertionError):
        R.certify(C, rows, np.array([1, 0]), u, v)
    rows, cols, u, v = R.linear_sum_assignment(C.T, return_duals=True)  # transposed: the duals come back in C's orientation
    assert rows.tolist() == [0, 1] and cols.tolist() == [0, 1] and len(u) == 3 and len(v) == 2
    assert R.certify(C.T, rows, cols, u, v) == 0.0
