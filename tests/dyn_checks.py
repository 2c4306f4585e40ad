"""What the synthesis sweep shares (tests/test_dyn_cases.py on the CPU, tests/test_gpu_dyn_sweep.py on the device): the
named case table, the crafted-instance generator, the CPU restatement of the five flag predicates, the reference
(``oracle.dyn_oracle`` on the CPU, selections applied by indexing) and ``paths``: the host dispatch of
mal_amd/csrc/mal_dyn.hip restated in Python, naming the kernels and branches a run of a case takes.

Every comparison of the sweep is bit equality: images are multiples of 1/256 in [0, 1) (a sum of <= 64 of them is exact
in fp32 in any order), cotangents multiples of 1/64 with |.| < 8 (a gradient element sums <= 2 + 2 x 64 of them: exact).

A case is a batch for ``BatchSynthesisFn``: ``items`` gives, per listed sample, the number of instances (or "crafted":
the instances of ``crafted_boxes``), optionally with a selection kind; ``DynamicInstanceFn`` runs on the first item."""
import functools
import zlib

import numpy as np
import torch

from oracle import dyn_oracle as D

MASK_BYTES = (1, 2, 0x40, 0x80, 0xff)
K_EXT_CHUNKS, K_DYN_BATCH, MAX_INSTANCES = 8, 16, 64  # kExtChunks, kDynBatch (mal_dyn.hip), MAL_MAX_INSTANCES (mal_hip.h)
FORMS = ("out", "scratch", "snapshot")  # the backward: out of place, in place through scratch, region snapshots


# ---------------------------------------------------------------- instances with prescribed extents
def box_masks(H, W, boxes, rng, density=0.7):
    """boxes: per instance ((top, low, left, right) of "last" or None, the same for "next") -> two (num,H,W) bool tensors.
    The two corners (top, left) and (low, right) are set, the interior is random: for top, left >= 1 the extents the
    kernels derive are the prescribed ones, so the displacement is chosen, not drawn.  A fifth element of a box is its own
    density (1.0: a full box)."""
    out = [torch.zeros(len(boxes), H, W, dtype=torch.bool) for _ in range(2)]
    for i, pair in enumerate(boxes):
        for which, box in enumerate(pair):
            if box is None:
                continue
            top, low, left, right = box[:4]
            assert 0 <= top <= low < H and 0 <= left <= right < W, (box, H, W)
            blob = torch.from_numpy(rng.random((low - top + 1, right - left + 1)) < (box[4] if len(box) > 4 else density))
            blob[0, 0] = blob[-1, -1] = True
            out[which][i, top:low + 1, left:right + 1] = blob
    return out[0], out[1]


def moved(box, a, b, c, d):
    """the box whose low / top / right / left differ from ``box``'s by a / b / c / d"""
    top, low, left, right = box
    return (box, (top + b, low + a, left + d, right + c))


def crafted_boxes(H, W):
    """instances for a canvas of at least 20 x 36 that walk the edges of the displacement rule and of the copies"""
    assert H >= 20 and W >= 36
    full = lambda *b: b
    return [
        moved(full(6, 10, 4, 9), 4, -4, 3, 1),        # rows: a tie a = -b -> the first, 4 / 2 = 2; columns 3 / 2 -> 2
        moved(full(3, 7, 14, 18), 1, 0, -1, 0),       # halves +1, -1 -> 0, -0
        moved(full(10, 16, 20, 25), -3, 1, 5, 2),     # -3 / 2 -> -2, 5 / 2 -> 2
        moved(full(2, 6, 26, 33), 2, 5, -5, -3),      # 5 / 2 -> 2, -5 / 2 -> -2
        moved(full(12, 15, 6, 12), 3, -3, -3, 3),     # ties both ways: (3, -3) -> 3 -> 2; (-3, 3) -> -3 -> -2
        (full(1, 12, 1, 6), full(1, 4, 3, 8)),        # dx = -4: the "last" copy leaves through the top; dy = 1
        (full(8, H - 1, 28, 33), full(16, H - 1, 26, 31)),   # dx = 4: through the bottom; dy = -1
        (full(5, 9, 1, 12), full(5, 9, 1, 4)),        # dy = -4: through the left border
        (full(14, 17, W - 12, W - 1), full(14, 17, W - 4, W - 1)),  # dy = 4: through the right border
        (full(3, 5, 10, 13), full(3, 5, 16, 19)),     # dy = 3
        (full(16, 18, 16, 19), full(16, 18, 10, 13)),  # dy = -3
        (full(7, 9, 20, 22), None),                   # vanished in "next"
        (full(0, 0, 5, 9), full(0, 0, 6, 11)),        # visible in row 0 only: no extents at all
        (full(3, 6, 0, 0), full(4, 8, 0, 0)),         # in column 0 only: rows are seen, columns are not
        (None, None),                                 # an all-empty pair
        (full(9, 13, 13, 18), full(11, 15, 13, 18)),  # three instances on top of each other
        (full(9, 13, 13, 18), full(11, 15, 13, 18)),
        (full(9, 13, 13, 18), full(11, 15, 13, 18)),
        (full(11, 14, 30, 33), full(11, 14, 24, 27)),  # dy = -3 at a second place (|d| = 3 survives replace)
        # column 0 TOGETHER with other columns, full boxes: left is 1 (column 0 is invisible), so (right, left) move by (2, 5)
        # and dy = 5 / 2 -> 2; with column 0 visible it were (2, 6) -> 3.  The same for row 0: dx = 2, not 3.
        (full(17, 19, 0, 6, 1.0), full(17, 19, 6, 8, 1.0)),
        (full(0, 4, 34, 35, 1.0), full(6, 6, 34, 35, 1.0)),
    ]


def random_boxes(H, W, num, rng):
    def box():
        top, left = int(rng.integers(0, H)), int(rng.integers(0, W))
        return (top, int(rng.integers(top, min(H, top + max(2, H // 2)))), left, int(rng.integers(left, min(W, left + max(2, W // 2)))))
    out = []
    for _ in range(num):
        r = rng.random()
        out.append((box(), None) if r < 0.06 else ((None, box()) if r < 0.12 else (box(), box())))
    return out


# ---------------------------------------------------------------- the case table
def _c(H, W, items, **kw):
    d = dict(H=H, W=W, items=list(items), C=3, replace=False, B=None, listed=None, mask_off=None, img_off=0, ct_off=0,
             bytes=False, blocks=(1,))
    d.update(kw)
    return d


CASES = {
    # the scalar kernels: W % 4 != 0
    "scalar_2x2": _c(2, 2, [1]),
    "scalar_5x3": _c(5, 3, [2, 3], B=3, listed=(2, 0)),
    "scalar_21x37_crafted": _c(21, 37, ["crafted", 3], B=3, listed=(0, 2)),
    "scalar_21x37_crafted_replace": _c(21, 37, ["crafted"], replace=True),
    "scalar_21x37_bytes": _c(21, 37, ["crafted", 4], bytes=True),
    # quads at wmax = 0 (W = 4); H < 8 leaves empty bands; 32x4: the 16-byte scan of the scalar extents
    "quad_2x4": _c(2, 4, [2]),
    "quad_32x4": _c(32, 4, [3, 1]),
    "quad_12x8_a_load_spans_two_rows": _c(12, 8, [3, 2]),
    "quad_9x8_both_scans": _c(9, 8, [2, 2]),
    "quad_16x24": _c(16, 24, [4, 2], B=3, listed=(1, 2)),
    "quad_24x40_crafted": _c(24, 40, ["crafted", 2]),
    "quad_24x40_crafted_replace": _c(24, 40, ["crafted"], replace=True),
    "quad_24x40_bytes": _c(24, 40, ["crafted", 3], bytes=True),
    # W % 16 == 0: extents16 (empty bands at 3x16), both workgroup sizes
    "wide_3x16": _c(3, 16, [2, 3], blocks=(1, 0)),
    "wide_8x16": _c(8, 16, [3, 1], blocks=(1, 0)),
    "wide_40x32_copies_cross_a_workgroup": _c(40, 32, [5, 4], blocks=(1, 0)),
    "wide_24x48_crafted": _c(24, 48, ["crafted", 2], blocks=(1, 0)),
    "wide_24x48_crafted_replace_bytes": _c(24, 48, ["crafted"], replace=True, bytes=True),
    "wide_48x80": _c(48, 80, [7]),
    # alignment: torch allocations are 512-byte aligned, offsets into a larger buffer set the alignment
    "mask_plus1_24x48": _c(24, 48, [3, 2], mask_off=(1, 1)),
    "mask_plus4_24x48": _c(24, 48, [3, 2], mask_off=(4, 4)),
    "mask_plus1_24x40_bytes": _c(24, 40, ["crafted"], mask_off=(1,), bytes=True),
    "img_plus1_24x40": _c(24, 40, [4, 2], img_off=1),
    "ct_plus1_24x40": _c(24, 40, [4, 2], ct_off=1),
    "img_and_ct_plus1_24x48": _c(24, 48, [3], img_off=1, ct_off=1),
    "one_item_alone_misaligned_8x16": _c(8, 16, [2, 2, 2], mask_off=(0, 1, 0)),
    # sizes
    "num17_16x24": _c(16, 24, [17]),
    "num64_24x40": _c(24, 40, [64]),
    "num64_21x37": _c(21, 37, [64]),
    "ragged_16x32": _c(16, 32, [1, 17, 3, 64], B=5, listed=(4, 0, 1, 3)),
    "items17_8x16": _c(8, 16, [1 + k % 3 for k in range(17)]),
    "items33_8x16": _c(8, 16, [1 + k % 4 for k in range(33)], B=34, listed=tuple(range(33, 0, -1))),
    "items17_5x3": _c(5, 3, [1 + k % 2 for k in range(17)]),
    "c1_24x40": _c(24, 40, [4, 2], C=1),
    "c2_24x48": _c(24, 48, [4], C=2),
    "c4_24x40": _c(24, 40, ["crafted"], C=4),
    "c4_5x3": _c(5, 3, [2], C=4),
    # int64 selections applied inside the kernels
    "sel_permutes_24x40": _c(24, 40, [(5, "perm"), (3, "perm")]),
    "sel_shorter_16x24": _c(16, 24, [(3, "short"), 2]),
    "sel_rows_differ_24x48": _c(24, 48, [(4, "rows")]),
    "sel_rows_differ_21x37": _c(21, 37, [(4, "rows"), (2, "short")]),
}


def _item_spec(it):
    num, sel = it if isinstance(it, tuple) else (it, None)
    return num, sel


@functools.lru_cache(maxsize=None)
def make(name):
    """-> dict: the spec plus, per item, masks (uint8 or bool, (rows,H,W)), selections (int64 or None) and the SELECTED bool
    masks; images cl, cn (B,C,H,W) and cotangents wl, wn.  Seeded from the name."""
    spec = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    H, W, C = spec["H"], spec["W"], spec["C"]
    n_items = len(spec["items"])
    listed = tuple(spec["listed"]) if spec["listed"] is not None else tuple(range(n_items))
    B = spec["B"] or n_items
    assert len(listed) == n_items and len(set(listed)) == n_items and max(listed) < B
    items = []
    for k, it in enumerate(spec["items"]):
        num, sel = _item_spec(it)
        boxes = crafted_boxes(H, W) if num == "crafted" else random_boxes(H, W, num, rng)
        ml, mn = box_masks(H, W, boxes, rng)
        num = len(boxes)
        sel_l = sel_n = None
        full_l, full_n = ml, mn
        if sel is not None:
            extra_l, extra_n = {"perm": (0, 0), "short": (2, 2), "rows": (1, 3)}[sel]
            rows_l, rows_n = num + extra_l, num + extra_n
            pl, pn = rng.permutation(rows_l), rng.permutation(rows_n)
            sel_l, sel_n = torch.from_numpy(pl[:num].copy()), torch.from_numpy(pn[:num].copy())
            full_l = box_masks(H, W, random_boxes(H, W, rows_l, rng), rng)[0]
            full_n = box_masks(H, W, random_boxes(H, W, rows_n, rng), rng)[1]
            full_l[sel_l], full_n[sel_n] = ml, mn
        if spec["bytes"]:
            val = lambda m: torch.from_numpy(rng.choice(np.array(MASK_BYTES, dtype=np.uint8), size=tuple(m.shape))) * m.to(torch.uint8)
            full_l, full_n = val(full_l), val(full_n)
        items.append(dict(b=listed[k], num=num, masks=(full_l, full_n), sel=(sel_l, sel_n), selected=(ml, mn),
                          mask_off=(spec["mask_off"][k] if spec["mask_off"] else 0)))
    img = lambda: torch.from_numpy(rng.integers(0, 256, (B, C, H, W)).astype(np.float32) / 256)
    ct = lambda: torch.from_numpy(np.clip(np.round(rng.standard_normal((B, C, H, W)) * 64), -511, 511).astype(np.float32) / 64)
    d = dict(spec)
    d.update(name=name, B=B, listed=listed, items=items, cl=img(), cn=img(), wl=ct(), wn=ct())
    return d


# ---------------------------------------------------------------- the reference
def flags_of(ml, mn, replace):
    """the five predicates of a pixel as the flag byte of the kernels (mal_dyn.hip, DynParams.flags), on the CPU:
    bit 0 region = or_i (last_i | next_i);  bit 1 / 2: some shifted copy of "last" / "next" lands here;
    bit 3 / 4: or_i (last_i & ~next_i) / or_i (next_i & ~last_i)"""
    dx, dy = D.deltas(ml, mn, replace)
    any_l = torch.zeros(ml.shape[1:], dtype=torch.bool)
    any_n = torch.zeros(ml.shape[1:], dtype=torch.bool)
    for i in range(ml.shape[0]):
        any_l |= D._shift(ml[i], int(dx[i]), int(dy[i]), False)
        any_n |= D._shift(mn[i], -int(dx[i]), -int(dy[i]), False)
    region, bg_l, bg_n = (ml | mn).any(0), (ml & ~mn).any(0), (mn & ~ml).any(0)
    f = region.int() | (any_l.int() << 1) | (any_n.int() << 2) | (bg_l.int() << 3) | (bg_n.int() << 4)
    return f.to(torch.uint8)


@functools.lru_cache(maxsize=None)
def reference(name):
    """per item: ori_last / ori_next, the gradients of both images for (both cotangents, "last" only, "next" only), the
    flag bytes; computed once and shared"""
    d = make(name)
    out = []
    for it in d["items"]:
        b = it["b"]
        ml, mn = it["selected"]
        il, inx = d["cl"][b].clone().requires_grad_(True), d["cn"][b].clone().requires_grad_(True)
        ol, on = D.generate_dynamic_instance(ml, mn, il, inx, d["replace"])
        sl, sn = (ol * d["wl"][b]).sum(), (on * d["wn"][b]).sum()
        g_both = torch.autograd.grad(sl + sn, [il, inx], retain_graph=True)
        g_last = torch.autograd.grad(sl, [il, inx], retain_graph=True, allow_unused=True)
        g_next = torch.autograd.grad(sn, [il, inx], allow_unused=True)
        z = lambda t: torch.zeros_like(il) if t is None else t
        out.append(dict(ol=ol.detach(), on=on.detach(), g_both=g_both, g_last=tuple(map(z, g_last)), g_next=tuple(map(z, g_next)),
                        flags=flags_of(ml, mn, d["replace"])))
    return out


# ---------------------------------------------------------------- the dispatch of mal_dyn.hip, restated
def _extents_paths(H, W, mask_offs, rows, small_blocks):
    """dyn_fwd_chunk's choice of the extents kernel for one chunk of items, and the scan each workgroup of
    dyn_extents_kernel takes (the base of instance row r is mask + r H W)"""
    if W % 16 == 0 and all(o % 16 == 0 for o in mask_offs):
        return {"extents16@256" if small_blocks else "extents16@1024"}
    out = set()
    band = (H + K_EXT_CHUNKS - 1) // K_EXT_CHUNKS
    for off, item_rows in zip(mask_offs, rows):
        for r in item_rows:
            for chunk in range(K_EXT_CHUNKS):
                r_lo = chunk * band
                r_hi = min(r_lo + band, H)
                if r_hi <= r_lo:
                    out.add("extents:empty_band")
                    continue
                k_lo, hw = r_lo * W, r_hi * W
                wide = hw % 16 == 0 and k_lo % 16 == 0 and (off + r * H * W) % 16 == 0
                out.add("extents:scan16" if wide else "extents:bytes")
    return out


def paths(name, api, form="out", prefilled=False, small_blocks=1):
    """the kernels, branches and input traits of one run of a case: ``api`` "instance" (DynamicInstanceFn on the first item,
    the selection applied by indexing) or "batch" (BatchSynthesisFn on all items)."""
    d = make(name)
    H, W, C = d["H"], d["W"], d["C"]
    items = d["items"][:1] if api == "instance" else d["items"]
    out = set()
    img16 = (4 * d["img_off"]) % 16 == 0          # images (and, prefilled, nothing else: the outputs are fresh allocations)
    ct16 = (4 * d["ct_off"]) % 16 == 0
    fwd_quads, bwd_quads = [], []
    for o in range(0, len(items), K_DYN_BATCH):
        chunk = items[o:o + K_DYN_BATCH]
        offs = [it["mask_off"] for it in chunk]
        if api == "instance":
            rows = [range(it["num"]) for it in chunk]
        else:
            rows = [sorted(set((it["sel"][0].tolist() if it["sel"][0] is not None else list(range(it["num"])))
                               + (it["sel"][1].tolist() if it["sel"][1] is not None else list(range(it["num"]))))) for it in chunk]
        out |= _extents_paths(H, W, offs, rows, small_blocks)
        masks4 = all(x % 4 == 0 for x in offs)
        # flags: a fresh (B,H,W) byte map, sample b at b H W -- 4-byte aligned whenever W % 4 == 0
        fq = W % 4 == 0 and C == 3 and masks4 and img16
        # backward: g_ori = the cotangent (a snapshot: fresh, aligned), g_img = fresh / the cotangent itself in place
        g_ori16 = True if form == "snapshot" else ct16
        g_img16 = True if form == "out" else ct16
        bq = W % 4 == 0 and C == 3 and masks4 and g_ori16 and g_img16
        fwd_quads.append(fq)
        bwd_quads.append(bq)
        out.add(("fwd4" if fq else "fwd") + (":prefilled" if prefilled else ""))
        out.add(("bwd4:" if bq else "bwd:") + form)
        if fq and not bq:
            out.add("fwd4+bwd")
        if bq and not fq:
            out.add("fwd+bwd4")
        if o > 0:
            out.add("second_chunk")
    # traits of the inputs
    nums = [it["num"] for it in items]
    out |= {"num=%d" % n for n in nums if n in (1, 17, 64)}
    if api == "batch":
        if len(set(nums)) > 1:
            out.add("ragged_num")
        if (H, W) == (8, 16) and len(items) in (17, 33):
            out.add("items=%d@8x16" % len(items))
        offs = [it["mask_off"] for it in items]
        if sum(1 for x in offs if x % 4) == 1 and len(items) > 1:
            out.add("one_item_alone_misaligned")
        for it in items:
            sl, sn = it["sel"]
            if sl is not None:
                rl, rn = it["masks"][0].shape[0], it["masks"][1].shape[0]
                if rl != rn:
                    out.add("sel:rows_differ")
                if len(sl) < rl:
                    out.add("sel:shorter")
                if len(sl) == rl and sl.tolist() != list(range(rl)):
                    out.add("sel:permutes")
        if d["B"] > len(items):
            out.add("unlisted_samples")
    out |= {"mask+%d" % x for it in items for x in (it["mask_off"],) if x in (1, 4)}
    if d["img_off"] == 1:
        out.add("img+1float")
    if d["ct_off"] == 1:
        out.add("ct+1float")
    out.add("C=%d" % C)
    if W == 4:
        out.add("W=4")
    if H < 8:
        out.add("H<8")
    if d["bytes"]:
        out.add("mask_bytes")
    return out


def runs():
    """every (case, api, form, prefilled, small_blocks) the device sweep executes; prefilled exists for the batch node only"""
    out = []
    for name, spec in CASES.items():
        for sb in spec["blocks"]:
            out.append((name, "instance", "out", False, sb))
            for form in FORMS:
                for pre in (False, True):
                    out.append((name, "batch", form, pre, sb))
    return out


REQUIRED_PATHS = (
    "extents16@256", "extents16@1024", "extents:scan16", "extents:bytes", "extents:empty_band",
    "fwd4", "fwd4:prefilled", "fwd", "fwd:prefilled",
    "bwd4:out", "bwd4:scratch", "bwd4:snapshot", "bwd:out", "bwd:scratch", "bwd:snapshot",
    "fwd4+bwd", "fwd+bwd4", "second_chunk",
    "mask+1", "mask+4", "img+1float", "ct+1float", "one_item_alone_misaligned",
    "num=1", "num=17", "num=64", "ragged_num", "items=17@8x16", "items=33@8x16", "C=1", "C=2", "C=3", "C=4",
    "sel:permutes", "sel:shorter", "sel:rows_differ", "W=4", "H<8", "mask_bytes", "unlisted_samples",
)


# ---------------------------------------------------------------- the edges the table must contain, found by computation
def _visible_extents(m):
    """low, top, right, left of one (H,W) mask if row 0 and column 0 counted like any other (what the rule is NOT)"""
    r, c = torch.nonzero(m.any(1)).flatten(), torch.nonzero(m.any(0)).flatten()
    return torch.tensor([int(r.max()) if len(r) else 0, int(r.min()) if len(r) else 0,
                         int(c.max()) if len(c) else 0, int(c.min()) if len(c) else 0])


def _pick(a, b):
    s = b if abs(b) > abs(a) else a
    return int(torch.round(torch.tensor(s / 2.0)))


def edges(name):
    """the edges of the displacement rule and of the copies that the SELECTED instances of a case contain"""
    d = make(name)
    H, W = d["H"], d["W"]
    out = set()
    for it in d["items"]:
        ml, mn = it["selected"]
        el, en = D.extents(ml), D.extents(mn)
        dx, dy = D.deltas(ml, mn, False)
        rx, ry = D.deltas(ml, mn, d["replace"])
        for i in range(ml.shape[0]):
            for a, b, axis in ((int(en[i, 0] - el[i, 0]), int(en[i, 1] - el[i, 1]), "row"),
                               (int(en[i, 2] - el[i, 2]), int(en[i, 3] - el[i, 3]), "col")):
                if a == -b and a != 0:
                    out.add("pick_tie")
                s = b if abs(b) > abs(a) else a
                if abs(s) in (1, 3, 5):
                    out.add("half%+d" % s)
            if d["replace"]:
                for v in (int(dx[i]), int(dy[i])):
                    if abs(v) in (2, 3):
                        out.add("replace|d|=%d" % abs(v))
            if int(dy[i]) != 0:
                out.add("dy%%4=%d%s" % (abs(int(dy[i])) % 4, "+" if dy[i] > 0 else "-"))
            # a copy clipped at a border: a mask pixel whose destination lies outside
            for m, sx, sy in ((ml[i], int(rx[i]), int(ry[i])), (mn[i], -int(rx[i]), -int(ry[i]))):
                rr, cc = torch.nonzero(m, as_tuple=True)
                if len(rr):
                    if int((rr + sx).min()) < 0:
                        out.add("clipped_top")
                    if int((rr + sx).max()) >= H:
                        out.add("clipped_bottom")
                    if int((cc + sy).min()) < 0:
                        out.add("clipped_left")
                    if int((cc + sy).max()) >= W:
                        out.add("clipped_right")
            if bool(ml[i].any()) and not bool(mn[i].any()):
                out.add("vanished")
            if not bool(ml[i].any()) and not bool(mn[i].any()):
                out.add("all_empty_pair")
            for m in (ml[i], mn[i]):
                if bool(m.any()) and not bool(m[1:].any()):
                    out.add("row0_only")
                if bool(m.any()) and not bool(m[:, 1:].any()):
                    out.add("col0_only")
        # an instance whose displacement depends on row / column 0 being invisible to the extents
        vis = lambda m: torch.stack([_visible_extents(m[i]) for i in range(m.shape[0])])
        vl, vn = vis(ml), vis(mn)
        for i in range(ml.shape[0]):
            if _pick(int(vn[i, 0] - vl[i, 0]), int(vn[i, 1] - vl[i, 1])) != int(dx[i]):
                out.add("row0_masking_decides")
            if _pick(int(vn[i, 2] - vl[i, 2]), int(vn[i, 3] - vl[i, 3])) != int(dy[i]):
                out.add("col0_masking_decides")
        copies = torch.zeros(H, W, dtype=torch.int64)
        for i in range(ml.shape[0]):
            copies += D._shift(ml[i], int(rx[i]), int(ry[i]), False).long()
        if int(copies.max()) >= 3:
            out.add("3_overlapping_copies")
        if d["bytes"]:
            seen = set(np.unique(torch.cat([it["masks"][0].flatten(), it["masks"][1].flatten()]).numpy()).tolist()) - {0}
            if seen == set(MASK_BYTES):
                out.add("mask_bytes_all_five")
    return out


REQUIRED_EDGES = ("pick_tie", "half+1", "half-1", "half+3", "half-3", "half+5", "half-5", "replace|d|=2", "replace|d|=3",
                  "clipped_top", "clipped_bottom", "clipped_left", "clipped_right",
                  "dy%4=0+", "dy%4=1+", "dy%4=2+", "dy%4=3+", "dy%4=0-", "dy%4=1-", "dy%4=2-", "dy%4=3-",
                  "3_overlapping_copies", "vanished", "row0_only", "col0_only", "all_empty_pair", "mask_bytes_all_five",
                  "row0_masking_decides", "col0_masking_decides")
