"""CPU: the synthesis sweep's case table (tests/dyn_checks.py) reaches every kernel and branch of mal_dyn.hip's host
dispatch, holds every edge of the displacement rule and of the copies, and its inputs make bit equality a fair demand.
Also the two reference-made fixtures that pin the summation-order contract of ``oracle.dyn_oracle``."""
import numpy as np
import pytest
import torch

from oracle import dyn_oracle as D
from tests import dyn_checks as K
from tests import golden_io as G


def test_the_table_reaches_every_kernel_and_branch():
    seen = {}
    for run in K.runs():
        for p in K.paths(*run):
            seen.setdefault(p, run)
    missing = [p for p in K.REQUIRED_PATHS if p not in seen]
    assert not missing, missing
    # the shapes the design names are in the table
    shapes = {(c["H"], c["W"]) for c in K.CASES.values()}
    assert {(2, 2), (5, 3), (21, 37), (2, 4), (32, 4), (12, 8), (9, 8), (16, 24), (3, 16), (8, 16), (40, 32)} <= shapes
    assert max(h * w for h, w in shapes) <= 48 * 80
    for name in ("wide_3x16", "wide_8x16"):
        assert K.CASES[name]["blocks"] == (1, 0)


def test_named_shapes_take_the_branches_they_are_in_the_table_for():
    p = lambda name, **kw: K.paths(name, "batch", **kw)
    assert {"extents:scan16", "fwd4", "W=4"} <= p("quad_32x4") and "extents:bytes" not in p("quad_32x4")
    assert {"extents:bytes", "extents:empty_band", "fwd4", "H<8"} <= p("quad_2x4")
    assert p("quad_12x8_a_load_spans_two_rows") >= {"extents:scan16"} and "extents:bytes" not in p("quad_12x8_a_load_spans_two_rows")
    assert {"extents:scan16", "extents:bytes"} <= p("quad_9x8_both_scans")
    assert "extents:scan16" in p("quad_16x24") and "extents:bytes" not in p("quad_16x24")
    assert {"extents16@256", "extents:empty_band"} & p("wide_3x16") == {"extents16@256"}
    assert "extents16@1024" in p("wide_8x16", small_blocks=0)
    for name in ("scalar_2x2", "scalar_5x3", "scalar_21x37_crafted"):
        assert {"fwd", "bwd:out"} <= p(name) and not {"fwd4", "bwd4:out"} & p(name)
    # the misaligned fallbacks at W % 4 == 0
    assert {"extents:bytes", "fwd", "bwd:scratch"} <= p("mask_plus1_24x48", form="scratch")
    assert {"extents:bytes", "fwd4", "bwd4:snapshot"} <= p("mask_plus4_24x48", form="snapshot")
    assert "fwd+bwd4" in p("img_plus1_24x40") and "fwd4+bwd" in p("ct_plus1_24x40")
    assert "bwd:snapshot" in p("ct_plus1_24x40", form="snapshot")  # (the snapshot is aligned, the buffer written is not)
    assert {"fwd", "one_item_alone_misaligned"} <= p("one_item_alone_misaligned_8x16")
    assert "second_chunk" in p("items17_8x16") and "second_chunk" in p("items33_8x16") and "second_chunk" in p("items17_5x3")
    for c, name in ((1, "c1_24x40"), (2, "c2_24x48"), (4, "c4_24x40")):
        assert {"C=%d" % c, "fwd", "bwd:out"} <= p(name)


def test_the_table_holds_every_edge():
    seen = {}
    for name in K.CASES:
        for e in K.edges(name):
            seen.setdefault(e, name)
    missing = [e for e in K.REQUIRED_EDGES if e not in seen]
    assert not missing, missing
    # row / column 0 together with others, designed and not drawn: in the crafted set under every extents kernel
    for name in ("scalar_21x37_crafted", "quad_24x40_crafted", "wide_24x48_crafted", "wide_24x48_crafted_replace_bytes"):
        assert {"row0_masking_decides", "col0_masking_decides"} <= K.edges(name), name


def test_crafted_instances_have_the_prescribed_displacements():
    d = K.make("quad_24x40_crafted")
    ml, mn = d["items"][0]["selected"]
    dx, dy = D.deltas(ml, mn, False)
    want = [(2, 2), (0, 0), (-2, 2), (2, -2), (2, -2), (-4, 1), (4, -1), (0, -4), (0, 4), (0, 3), (0, -3)]
    assert list(zip(dx.tolist(), dy.tolist()))[:len(want)] == want
    rx, ry = D.deltas(ml, mn, True)
    assert rx.tolist()[:5] == [0, 0, 0, 0, 0] and ry.tolist()[7:11] == [-4, 4, 3, -3]


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_inputs_make_bit_equality_fair(name):
    """images are multiples of 1/256 in [0, 1), cotangents multiples of 1/64 below 8: every sum the kernels or the oracle
    form is exact in fp32 whatever the order; at most MAL_MAX_INSTANCES instances per item"""
    d = K.make(name)
    for t in (d["cl"], d["cn"]):
        assert float(t.min()) >= 0 and float(t.max()) < 1 and torch.equal(t * 256, torch.round(t * 256))
    for t in (d["wl"], d["wn"]):
        assert float(t.abs().max()) < 8 and torch.equal(t * 64, torch.round(t * 64))
    for it in d["items"]:
        assert 1 <= it["num"] <= K.MAX_INSTANCES
        for full, sel, chosen in zip(it["masks"], it["sel"], it["selected"]):
            picked = full if sel is None else full[sel]
            assert torch.equal(picked != 0, chosen)


def test_the_flag_restatement_agrees_with_the_oracle_where_the_oracle_shows_it():
    """the five predicates decide the oracle's output: rebuilding the output from the flags and plain sums gives its bits"""
    for name in ("quad_24x40_crafted", "scalar_21x37_crafted_replace", "num17_16x24"):
        d, ref = K.make(name), K.reference(name)
        it, r = d["items"][0], ref[0]
        ml, mn = it["selected"]
        il, inx = d["cl"][it["b"]], d["cn"][it["b"]]
        dx, dy = D.deltas(ml, mn, d["replace"])
        acc = torch.zeros_like(il)
        for i in range(ml.shape[0]):
            acc = acc + D._shift(ml[i], int(dx[i]), int(dy[i]), False) * D._shift(il, int(dx[i]), int(dy[i]), 0.0)
        f = r["flags"].int()
        want = torch.where((f & 1).bool(), torch.where((f & 2).bool(), acc, torch.where((f & 8).bool(), inx, il)), il)
        assert torch.equal(want, r["ol"])
        assert int(f.max()) < 32 and bool(((f & 1) == 0)[(f & 24) != 0].sum() == 0)


# ---------------------------------------------------------------- the order contract, pinned by the reference
def _load_order(tag):
    z = G.load(tag)
    ml, mn = torch.from_numpy(z["in/mask_last"]), torch.from_numpy(z["in/mask_next"])
    den = float(z["in/denominator"])
    il = torch.from_numpy(z["in/img_last"].astype(np.float32)) / den
    inx = torch.from_numpy(z["in/img_next"].astype(np.float32)) / den
    return z, ml, mn, il, inx


def test_crafted_edges_fixture_is_bit_exact_with_order_independent_sums():
    """the reference's own TorchScript functions on the crafted instances plus 20 overlapping ones, images k/256: every
    sum is exact whatever the order, and the oracle equals the reference bit for bit, gradients included"""
    z, ml, mn, il, inx = _load_order("dyn_edges_k256_24x40")
    assert ml.shape[0] == 20 + len(K.crafted_boxes(24, 40))
    for replace in (False, True):
        sfx = "_replace" if replace else ""
        a, b = il.clone().requires_grad_(True), inx.clone().requires_grad_(True)
        ol, on = D.generate_dynamic_instance(ml, mn, a, b, replace)
        assert np.array_equal(ol.detach().numpy(), z["out/ori_last" + sfx]) and np.array_equal(on.detach().numpy(), z["out/ori_next" + sfx])
        ct_l, ct_n = torch.from_numpy(z["in/ct_last"]), torch.from_numpy(z["in/ct_next"])
        gl, gn = torch.autograd.grad((ol * ct_l).sum() + (on * ct_n).sum(), [a, b])
        assert np.array_equal(gl.numpy(), z["out/g_img_last" + sfx]) and np.array_equal(gn.numpy(), z["out/g_img_next" + sfx])


def test_twenty_overlapping_copies_of_k255_images_differ_by_the_order_only():
    """20 overlapping copies of k/255 images: the reference's ``img_mv.sum(dim=0)`` is sequential up to 16 terms and cascaded
    above, the oracle (and the kernels) add in instance order.  Both are sums of n <= 20 non-negative fp32 terms formed by
    n - 1 rounded additions; the terms are non-negative and rounding is monotone, so no partial sum of either order exceeds
    that order's result, hence M = max(oracle, reference): each addition errs by at most half an ulp of a number <= M,
    |either - exact| <= (n - 1) ulp(M) / 2, and the two differ by at most (n - 1) ulp(M), ulp(M) = 2^(floor(log2 M) - 23).
    n is the number of copies on the pixel: the reference sums all 20 terms, zeros included (so its grouping is the
    cascaded one on every pixel), but an addition of zero is exact and only the n - 1 others count."""
    z, ml, mn, il, inx = _load_order("dyn_order_k255_n20_24x40")
    assert ml.shape[0] == 20
    il.requires_grad_(True), inx.requires_grad_(True)
    ol, on = D.generate_dynamic_instance(ml, mn, il, inx, False)
    # the gradients add cotangents (multiples of 1/64), not image values: exact in any order, bit for bit
    ct_l, ct_n = torch.from_numpy(z["in/ct_last"]), torch.from_numpy(z["in/ct_next"])
    gl, gn = torch.autograd.grad((ol * ct_l).sum() + (on * ct_n).sum(), [il, inx])
    assert np.array_equal(gl.numpy(), z["out/g_img_last"]) and np.array_equal(gn.numpy(), z["out/g_img_next"])
    ol, on = ol.detach(), on.detach()
    dx, dy = D.deltas(ml, mn, False)
    differs = 0
    for mine, ref, mask, sign in ((ol, z["out/ori_last"], ml, 1), (on, z["out/ori_next"], mn, -1)):
        n = torch.zeros(ml.shape[1:], dtype=torch.int64)
        for i in range(20):
            n += D._shift(mask[i], sign * int(dx[i]), sign * int(dy[i]), False).long()
        ref = torch.from_numpy(ref)
        largest = torch.maximum(ref.double().abs(), mine.double().abs()).clamp_min(2.0 ** -126)  # M of the docstring
        ulp = torch.exp2(torch.floor(torch.log2(largest)) - 23)
        bound = (n - 1).clamp_min(0).double() * ulp
        err = (mine.double() - ref.double()).abs()
        assert bool((err <= bound).all()), float((err - bound).max())
        assert torch.equal(mine[:, n <= 1], ref[:, n <= 1])  # nothing to add: the same bits
        assert int(n.max()) == 20
        differs += int((mine != ref).sum())
    assert differs > 0  # the fixture really exercises the order
