"""GPU: every case of tests/dyn_checks.py through ``DynamicInstanceFn`` and ``BatchSynthesisFn`` against
``oracle.dyn_oracle`` on the CPU -- outputs, gradients (both images, one image, one cotangent missing), all five flag bits,
prefilled against plain, the three backward forms.  Every comparison is bit equality on every pixel
(tests/test_dyn_cases.py shows why that is fair and that the table reaches every kernel and branch)."""
import pytest
import torch

from tests import dyn_checks as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="session", autouse=True)
def _built():
    from mal_amd import build
    build.build(verbose=False)


def place(t, off):
    """a contiguous device copy of ``t`` that starts ``off`` elements into a larger allocation (torch allocations are
    512-byte aligned: the offset IS the alignment)"""
    buf = torch.zeros(t.numel() + off + 64, dtype=t.dtype, device=DEV)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and (v.data_ptr() - buf.data_ptr()) == off * t.element_size() and buf.data_ptr() % 512 == 0
    return v


def eq(a, b):
    return torch.equal(a.detach().cpu(), b)


def with_blocks(small_blocks, fn):
    from mal_amd import _lib
    lib = _lib.load()
    assert lib.mal_set_option(b"dyn_small_blocks", small_blocks) == 0
    try:
        return fn()
    finally:
        lib.mal_set_option(b"dyn_small_blocks", 1)


INSTANCE_RUNS = [(n, sb) for (n, api, form, pre, sb) in K.runs() if api == "instance"]
BATCH_RUNS = [(n, sb) for (n, api, form, pre, sb) in K.runs() if api == "batch" and form == "out" and not pre]


@pytest.mark.parametrize("name,small_blocks", INSTANCE_RUNS, ids=lambda v: str(v))
def test_instance_node(name, small_blocks):
    with_blocks(small_blocks, lambda: _instance_node(name))


def _instance_node(name):
    from mal_amd import dyn_utils
    d, ref = K.make(name), K.reference(name)[0]
    it = d["items"][0]
    b = it["b"]
    # the selection applied by indexing; masks, images and cotangents at the offsets of the case
    full_l, full_n = it["masks"]
    sl, sn = it["sel"]
    ml = place(full_l if sl is None else full_l[sl], it["mask_off"])
    mn = place(full_n if sn is None else full_n[sn], it["mask_off"])
    il, inx = place(d["cl"][b], d["img_off"]).requires_grad_(True), place(d["cn"][b], d["img_off"]).requires_grad_(True)
    wl, wn = place(d["wl"][b], d["ct_off"]), place(d["wn"][b], d["ct_off"])
    ol, on = dyn_utils.DynamicInstanceFn.apply(ml, mn, il, inx, d["replace"])
    assert eq(ol, ref["ol"]) and eq(on, ref["on"])
    gl, gn = torch.autograd.grad([ol, on], [il, inx], [wl, wn], retain_graph=True)
    assert eq(gl, ref["g_both"][0]) and eq(gn, ref["g_both"][1])
    # one cotangent missing
    gl, gn = torch.autograd.grad([ol], [il, inx], [wl], retain_graph=True, allow_unused=True)
    assert eq(gl, ref["g_last"][0]) and eq(gn, ref["g_last"][1])
    gl, gn = torch.autograd.grad([on], [il, inx], [wn], retain_graph=True, allow_unused=True)
    assert eq(gl, ref["g_next"][0]) and eq(gn, ref["g_next"][1])
    # only one image requires grad: the other gradient pointer is null
    for k in (0, 1):
        a, c = il.detach().requires_grad_(k == 0), inx.detach().requires_grad_(k == 1)
        pl, pn = dyn_utils.DynamicInstanceFn.apply(ml, mn, a, c, d["replace"])
        (g,) = torch.autograd.grad([pl, pn], [a if k == 0 else c], [wl, wn])
        assert eq(g, ref["g_both"][k]), k
    # the flag bytes the node keeps for its backward
    flags = [t for t in ol.grad_fn.saved_tensors if t.dtype == torch.uint8 and tuple(t.shape) == (d["H"], d["W"])]
    assert len(flags) == 1 and eq(flags[0], ref["flags"])


def _batch_inputs(d):
    items = []
    for it in d["items"]:
        ml, mn = place(it["masks"][0], it["mask_off"]), place(it["masks"][1], it["mask_off"])
        if it["sel"][0] is None:
            items.append((it["b"], ml, mn))
        else:
            items.append((it["b"], ml, mn, it["sel"][0].to(DEV), it["sel"][1].to(DEV)))
    return items


@pytest.mark.parametrize("name,small_blocks", BATCH_RUNS, ids=lambda v: str(v))
def test_batch_node(name, small_blocks):
    with_blocks(small_blocks, lambda: _batch_node(name))


def _batch_node(name):
    from mal_amd import dyn_utils
    d, ref = K.make(name), K.reference(name)
    B, H, W = d["B"], d["H"], d["W"]
    items = _batch_inputs(d)
    cl, cn = place(d["cl"], d["img_off"]), place(d["cn"], d["img_off"])
    by_sample = {it["b"]: r for it, r in zip(d["items"], ref)}

    def expect(key, k, passthrough):
        return torch.stack([by_sample[b][key][k] if b in by_sample else passthrough[b] for b in range(B)])

    def expect_out(key, passthrough):
        return torch.stack([by_sample[b][key] if b in by_sample else passthrough[b] for b in range(B)])

    want_flags = torch.stack([by_sample[b]["flags"] if b in by_sample else torch.zeros(H, W, dtype=torch.uint8) for b in range(B)])
    zero = torch.zeros_like(d["wl"])
    for prefilled in (False, True):
        a_l, a_n = cl.detach().requires_grad_(True), cn.detach().requires_grad_(True)
        pre = (cl.clone(), cn.clone()) if prefilled else None
        sl, sn, flags = dyn_utils.BatchSynthesisFn.apply(a_l, a_n, items, d["replace"], pre)
        if prefilled:
            assert sl.data_ptr() == pre[0].data_ptr() and sn.data_ptr() == pre[1].data_ptr()
        assert eq(sl, expect_out("ol", d["cl"])) and eq(sn, expect_out("on", d["cn"])), prefilled
        assert eq(flags, want_flags), prefilled  # all five bits; zero for samples not listed
        # out of place: both cotangents, then one missing
        ct = [place(d["wl"], d["ct_off"]), place(d["wn"], d["ct_off"])]
        gl, gn = torch.autograd.grad([sl, sn], [a_l, a_n], ct, retain_graph=True)
        assert eq(gl, expect("g_both", 0, d["wl"])) and eq(gn, expect("g_both", 1, d["wn"])), prefilled
        gl, gn = torch.autograd.grad([sl], [a_l, a_n], ct[:1], retain_graph=True, allow_unused=True)
        assert eq(gl, expect("g_last", 0, d["wl"])) and eq(gn, expect("g_last", 1, zero)), prefilled
        gl, gn = torch.autograd.grad([sn], [a_l, a_n], ct[1:], retain_graph=True, allow_unused=True)
        assert eq(gl, expect("g_next", 0, zero)) and eq(gn, expect("g_next", 1, d["wn"])), prefilled
        # in place: through scratch, then from region snapshots (NaN outside the region: never read)
        for form in ("scratch", "snapshot"):
            ct = [place(d["wl"], d["ct_off"]), place(d["wn"], d["ct_off"])]
            assert all(t.data_ptr() % 16 == (4 * d["ct_off"]) % 16 for t in ct)
            reg = {t.data_ptr(): None for t in ct}
            if form == "snapshot":
                rg = (flags & 1).bool()[:, None].expand(B, d["C"], H, W)
                reg = {t.data_ptr(): torch.where(rg, t, torch.full_like(t, float("nan"))) for t in ct}
            dyn_utils.INPLACE_COTANGENTS.update(reg)
            try:
                hl, hn = torch.autograd.grad([sl, sn], [a_l, a_n], ct, retain_graph=True)
            finally:
                for k in reg:
                    dyn_utils.INPLACE_COTANGENTS.pop(k, None)
            assert hl.data_ptr() == ct[0].data_ptr() and hn.data_ptr() == ct[1].data_ptr()  # really in place
            assert eq(hl, expect("g_both", 0, d["wl"])) and eq(hn, expect("g_both", 1, d["wn"])), (prefilled, form)


def test_too_many_instances_and_one_row_are_refused():
    from mal_amd import dyn_utils
    from mal_amd._lib import MalError
    img = lambda H, W: torch.zeros(3, H, W, device=DEV)
    with pytest.raises(MalError):
        dyn_utils.DynamicInstanceFn.apply(torch.zeros(65, 8, 16, dtype=torch.bool, device=DEV),
                                          torch.zeros(65, 8, 16, dtype=torch.bool, device=DEV), img(8, 16), img(8, 16), False)
    with pytest.raises(MalError):
        dyn_utils.DynamicInstanceFn.apply(torch.zeros(1, 1, 16, dtype=torch.bool, device=DEV),
                                          torch.zeros(1, 1, 16, dtype=torch.bool, device=DEV), img(1, 16), img(1, 16), False)
    m = torch.zeros(65, 8, 16, dtype=torch.bool, device=DEV)
    with pytest.raises(MalError):
        dyn_utils.BatchSynthesisFn.apply(torch.zeros(1, 3, 8, 16, device=DEV), torch.zeros(1, 3, 8, 16, device=DEV), [(0, m, m)], False)
    # 64 is the limit and works (num64_* in the table)
