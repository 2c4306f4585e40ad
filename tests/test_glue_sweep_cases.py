"""CPU side of the glue sweep (tests/glue_sweep_cases.py, tests/test_gpu_glue_sweep.py): every decoder case is admitted by
mal_decoder_join_plan (pure host code) and has the property its band is named after, proven from the plan; the tables
hit every band; the carry rule of the strided odometer agrees with division at every unit every thread visits; the
restatement agrees with torch.autograd in fp64 at the small new cases; and the fp64 restatement of the encoder glue stays at
torch's own at the offset-statistics inputs."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import decoder_glue_restated as R
from tests import encoder_glue_cases as E
from tests import glue_sweep_cases as G
from tests.test_decoder_glue_cases import torch_composition


@pytest.fixture(scope="module", autouse=True)
def lib():
    from mal_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_plan_is_host_code_with_the_entry_points_checks(lib):
    f, b, per = (ctypes.c_int(-1) for _ in range(3))

    def plan(B=2, C=3, Cs=2, h=4, w=5, up=2, need_x=1, need_skip=1):
        return lib.mal_decoder_join_plan(B, C, Cs, h, w, up, need_x, need_skip, ctypes.byref(f), ctypes.byref(b), ctypes.byref(per))

    assert plan() == 0 and per.value > 0 and per.value % 4 == 0
    assert (f.value, b.value) == (-(-2 * 5 * 10 * 12 // per.value), -(-2 * 2 * 8 * 10 // per.value))
    for bad in (dict(up=0), dict(up=3), dict(B=0), dict(C=0), dict(h=0), dict(w=0), dict(B=-1), dict(Cs=-1), dict(up=1, h=1),
                dict(up=1, w=1), dict(need_x=2), dict(need_skip=-1), dict(B=64, C=512, h=256, w=256),
                dict(B=1, C=1, Cs=0, h=2 ** 30, w=2 ** 30), dict(B=2 ** 31 - 1, C=2 ** 31 - 1)):
        assert plan(**bad) == -1, bad
    assert lib.mal_decoder_join_plan(2, 3, 2, 4, 5, 2, 1, 1, None, None, None) == 0
    # nothing asked for, or gskip alone where there is no skip: no launch
    assert plan(need_x=0, need_skip=0) == 0 and b.value == 0 and f.value >= 1
    assert plan(Cs=0, need_x=0, need_skip=1) == 0 and b.value == 0


def test_the_grid_is_capped_and_the_backward_takes_the_larger_output():
    cap = G.cap()
    fwd, bwd, per = G.plan(G.TRAINING_SHAPE)
    n_out, nx, ns = G.sizes(G.TRAINING_SHAPE)
    assert fwd == bwd == cap and per % 4 == 0
    assert G.sweeps(n_out, fwd, per) == 12 and G.sweeps(nx, bwd, per) == 3  # what the workload launches at scale 0
    for case in G.SWEEP_CASES + R.CASES:
        fwd, bwd, per_ = G.plan(case)
        n_out, nx, ns = G.sizes(case)
        assert per_ == per
        assert fwd == min(cap, max(1, -(-n_out // per)))
        assert bwd == min(cap, max(1, -(-max(nx, ns) // per)))
        assert G.plan(case, True, False)[1] == min(cap, -(-nx // per))
        assert G.plan(case, False, True)[1] == (min(cap, -(-ns // per)) if ns else 0)


def test_every_old_case_stays_within_one_sweep():
    """why the sweep exists: no case of the table the kernels were merged with strides"""
    for case in R.CASES:
        assert all(s <= 1 for s, _ in G.profile(case).values()), case


def band_properties(case):
    """the bands a case fills, from the plan alone"""
    cap = G.cap()
    fwd, bwd, per = G.plan(case)
    n_out, nx, ns = G.sizes(case)
    p = G.profile(case)
    up = case[0]
    hit = set()
    if fwd == cap and n_out == cap * per:
        hit.add("fwd_exactly_one_sweep")
    if p["out"][0] == 2 and 0 < n_out - cap * per <= 4 * per:  # the second sweep is at most four workgroups' worth
        hit.add("fwd_one_sweep_and_a_short_tail")
    if p["out"][0] == 2 and all(d > 0 for d in p["out"][1]):
        hit.add("fwd_two_sweeps_every_stride_digit_nonzero")
    if p["out"][0] == 5 and p["out"][1][3] == 0 and p["gx"][0] >= 2 and up == 2:
        hit.add("fwd_five_sweeps_leading_digit_zero_gx_strided_up2")
    if p["gx"][0] >= 2 and up == 1:
        hit.add("gx_strided_up1")
    if p["gskip"][0] >= 2 and nx <= 0.1 * cap * per:
        hit.add("gskip_strided_gx_within_one_sweep")
    if p["gx"][0] >= 2 and p["gskip"][0] >= 2:
        hit.add("gx_and_gskip_strided")
    return hit


def test_every_strided_case_fills_its_band():
    for band, case in G.STRIDED.items():
        p = G.profile(case)
        print("%-52s %-28s elements %s sweeps %s digits of the forward's stride %s"
              % (band, R.case_id(case), G.sizes(case), tuple(v[0] for v in p.values()), p["out"][1]))
        assert band in band_properties(case), (band, case, p)
        assert max(G.sizes(case)) <= 9.1e6  # the smallest shape of a band, not the workload's
        if band in G.STATED_FWD_DIGITS:
            assert p["out"][1] == G.STATED_FWD_DIGITS[band]
    # in the backward of the shared grid, the smaller space strides by a stride of its own radices, and pruning changes the grid
    case = G.STRIDED["gskip_strided_gx_within_one_sweep"]
    assert G.plan(case, True, False)[1] < G.plan(case, True, True)[1] == G.plan(case, False, True)[1] == G.cap()
    case = G.STRIDED["fwd_five_sweeps_leading_digit_zero_gx_strided_up2"]
    assert G.profile(case)["gx"][1] != G.profile(case)["out"][1]


def test_the_strided_band_has_both_upsamplings_and_both_activations():
    strided = [c for c in G.SWEEP_CASES + R.CASES if any(s >= 2 for s, _ in G.profile(c).values())]
    assert {c[0] for c in strided} == {1, 2} and {c[1] for c in strided} == {0, 1}
    assert {c[0] for c in strided if G.profile(c)["gx"][0] >= 2} == {1, 2}
    assert any(c[4] == 0 for c in strided) and any(c[4] > 0 for c in strided)


def test_every_tail_residue_of_every_output_is_hit():
    seen = {"out": {}, "gx": {}, "gskip": {}}
    beyond_one_block = {"out": set(), "gx": set(), "gskip": set()}
    per = G.plan(G.TAILS[0])[2]
    for case in G.TAILS:
        assert all(s <= 1 for s, _ in G.profile(case).values())
        for name, n in zip(("out", "gx", "gskip"), G.sizes(case)):
            if n:
                seen[name].setdefault(n % 4, case)
                if n > per and n % 4:
                    beyond_one_block[name].add(n % 4)
    for name in seen:
        for res in (1, 2, 3):
            assert res in seen[name], (name, res)
            print("tail of %-5s residue %d: %s" % (name, res, R.case_id(seen[name][res])))
        assert beyond_one_block[name], name
    # what the old table reaches
    old = {name: {n % 4 for n in ns if n} for name, ns in zip(("out", "gx", "gskip"), zip(*(G.sizes(c) for c in R.CASES)))}
    print("residues of the old table:", old)


@pytest.mark.parametrize("case", G.SWEEP_CASES + [G.TRAINING_SHAPE], ids=R.case_id)
def test_the_carried_odometer_agrees_with_division(case):
    """every thread of the grid, every sweep, each of the three index spaces, for the full call and both pruned ones"""
    for need in ((True, True), (True, False), (False, True)):
        fwd, bwd, per = G.plan(case, *need)
        for name, (radices, n) in G.spaces(case).items():
            blocks = fwd if name == "out" else bwd
            if n == 0 or blocks == 0 or (name == "out" and need != (True, True)):
                continue
            stride = G.stride_digits(radices, blocks, per)
            assert all(d < r for d, r in zip(stride, radices))  # what one conditional subtraction per digit relies on
            flat = 4 * np.arange(blocks * per // 4, dtype=np.int64)
            flat = flat[flat < n]
            o = [d.copy() for d in G.odo_of(flat, radices)]
            visited = 0
            while flat.size:
                want = G.odo_of(flat, radices)
                assert all((a == b).all() for a, b in zip(o, want)), (name, need, int(flat[0]))
                assert (o[3] * radices[2] * radices[1] * radices[0] < n).all()
                visited += int(np.minimum(4, n - flat).sum())
                flat = flat + blocks * per
                keep = flat < n
                o = [d[keep] for d in G.odo_add(o, stride, radices)]
                flat = flat[keep]
            assert visited == n  # every element once


SMALL = [c for c in G.SWEEP_CASES if max(G.sizes(c)) <= 100000]


def test_the_small_cases_are_the_tails():
    assert SMALL == G.TAILS


@pytest.mark.parametrize("case", SMALL, ids=R.case_id)
def test_restatement_matches_torch_fp64_at_the_new_cases(case):
    up, elu, B, C, Cs, h, w = case
    x, skip, g = (None if a is None else a.astype(np.float64) for a in G.decoder_inputs(case, nonfinite=False))
    assert np.isfinite(x).all()
    tx = torch.from_numpy(x).requires_grad_(True)
    ts = torch.from_numpy(skip).requires_grad_(True) if skip is not None else None
    out = torch_composition(tx, ts, up, elu)
    assert np.abs(R.forward(x, skip, up, elu) - out.detach().numpy()).max() <= 1e-12
    out.backward(torch.from_numpy(g))
    gx, gskip = R.backward(g, x, up, elu)
    assert np.abs(gx - tx.grad.numpy()).max() <= 1e-12 * max(1.0, float(np.abs(tx.grad.numpy()).max()))
    if skip is not None:
        assert np.abs(gskip - ts.grad.numpy()).max() <= 1e-12


def test_planted_values_reach_the_inputs():
    with_all = 0
    for case in G.TAILS + [G.STRIDED["fwd_one_sweep_and_a_short_tail"]]:
        x = G.decoder_inputs(case)[0].reshape(-1)
        if x.size < 64:
            continue
        with_all += 1
        for v in R.PLANTED + G.PLANTED_FINITE + G.PLANTED_NONFINITE[:2]:
            assert (x.view(np.int32) == np.float32(v).view(np.int32)).any(), (case, v)
        assert np.isnan(x).sum() == 1
        assert np.isfinite(G.decoder_inputs(case, nonfinite=False)[0]).all()
    assert with_all >= 4
    assert G.DENORM > 0 and np.float32(G.DENORM) / np.float32(2) == 0


# ---------------------------------------------------------------------------------------------------------- encoder glue
def test_placed_tensors_are_contiguous_views_off_the_16_byte_grid():
    from mal_amd.glue import bn_join_fallback_reason
    import torch.nn as nn
    t = torch.arange(2 * 3 * 4 * 4, dtype=torch.float32).view(2, 3, 4, 4)
    for off in (0, 1, 2, 3):
        v = G.placed(t, off)
        assert torch.equal(v, t) and (v.data_ptr() % 16 == 0) == (off == 0)
        assert bn_join_fallback_reason(v, nn.BatchNorm2d(3), G.placed(t, (off + 1) % 4)) is None
    assert len(G.gradient_subsets()) == 15 and (False, True, False, False) in G.gradient_subsets()
    assert G.PLACED_SHAPE in E.TABLE_SHAPES and all(s in E.TABLE_SHAPES for s in G.PRUNED_SHAPES)
    assert all((H * W) % 4 == 0 for _, _, H, W in G.placed_shapes())  # V = 1 there comes from the addresses alone
    assert E.plan(*G.PRUNED_SHAPES[0])[0] > 1 and (27 * 33) % 4 != 0


@pytest.mark.parametrize("case", G.OFFSET_CASES, ids=E.case_id)
def test_offset_statistics_reference_stays_at_torchs_own(case):
    """the check of tests/test_encoder_glue_cases.py at the new inputs: the fp64 restatement against torch.autograd in fp64"""
    (B, C, H, W), mode, mean = case
    x, r, g, gamma, beta, rm, rv = (None if t is None else t.double() for t in G.offset_inputs(case))
    m, v = E.statistics(x)
    free = [c for c in range(C) if c != E.special_channels(C)[2]]
    assert float((m[free] - mean).abs().max()) < 0.01 and float((v[free].sqrt() / G.OFFSET_STD - 1).abs().max()) < 0.2
    relu = E.relu_of(mode)
    leaves = [t.clone().requires_grad_(True) for t in (x, gamma, beta)]
    lr = r.clone().requires_grad_(True) if r is not None else None
    trm, trv = rm.clone(), rv.clone()
    out = F.batch_norm(leaves[0], trm, trv, leaves[1], leaves[2], True, 0.1, E.EPS)
    out = out + lr if lr is not None else out
    out = F.relu(out) if relu else out
    out.backward(g)
    y, pre, xh = E.forward(x, r, gamma, beta, relu, m, v)
    dx, dr, dgamma, dbeta = E.backward(g, x, gamma, relu, m, v, mask=y > 0)
    erm, erv = E.running(rm, rv, m, v, B * H * W, 0.1)
    pairs = [(y, out), (dx, leaves[0].grad), (dgamma, leaves[1].grad), (dbeta, leaves[2].grad), (erm, trm), (erv, trv)]
    if lr is not None:
        pairs.append((dr, lr.grad))
    worst = max(E.l2rel(a, b) for a, b in pairs)
    print(E.case_id(case), "worst L2 rel of the restatement against torch.autograd in fp64: %.2e" % worst)
    assert worst <= 1e-9
