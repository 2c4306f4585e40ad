"""Instance matcher (mal_amd/matcher.py, mal_match) against the upstream-shaped path on the same box and inputs:
torch einsum costs on the device, two .cpu() syncs, a host assignment solver (tests/matcher_restated.py: numpy; scipy's
is used as well when it is installed), the intersection in Python and two host-to-device copies of the slices.

    python scripts/bench_matcher.py [calls]        # prints; profiles/matcher_bench.txt is a copy of the output

1. one call on fixture case e (192x640, 20 / 20 / 8 instances), HIP events around `calls` calls (>= 200);
2. dyn_utils.image_synthesis, eager, B=12 192x640, three instances per sample, with each matcher."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mal_amd import dyn_utils
from mal_amd.matcher import HungarianMatcher
from tests import matcher_restated as R

DEV = torch.device("cuda:0")
CALLS = max(int(sys.argv[1]) if len(sys.argv) > 1 else 200, 200)
try:
    from scipy.optimize import linear_sum_assignment as scipy_lsa
except ImportError:
    scipy_lsa = None


class Inst:
    def __init__(self, classes, masks, scores=None):
        self.pred_classes, self.pred_masks = classes, masks
        self.scores = scores if scores is not None else torch.full((len(classes),), 0.9)

    def __len__(self):
        return len(self.pred_classes)

    def __getitem__(self, sel):
        sel_d = sel.to(self.pred_masks.device) if torch.is_tensor(sel) else sel
        return Inst(self.pred_classes[sel_d], self.pred_masks[sel_d], self.scores[sel])


def upstream_shaped(lsa):
    """matcher.py:89-173 with the given host solver, masks as upstream gets them (float32 on the device)"""
    def dice(a, t):
        a = a.sigmoid().flatten(1)
        return 1 - (2 * torch.einsum("nc,mc->nm", a, t) + 1) / (a.sum(-1)[:, None] + t.sum(-1)[None, :] + 1)

    @torch.no_grad()
    def matcher(ins_n, ins_m, ins_0):
        n_0 = len(ins_0)
        t = ins_0.pred_masks.flatten(1).float()
        mats = []
        for ins in (ins_n, ins_m):
            cls = torch.where(ins.pred_classes.unsqueeze(1).repeat(1, n_0) == ins_0.pred_classes.repeat(len(ins), 1), 0, 1)
            mats.append((1 * cls + 1 * dice(ins.pred_masks.flatten(1).float(), t)).cpu())
        (idx_n, idx_0), (idx_m, idx_1) = lsa(mats[0].numpy()), lsa(mats[1].numpy())
        pairs, _ = R.intersect(idx_n, idx_0, idx_m, idx_1)
        dev = ins_n.pred_classes.device
        return (torch.as_tensor(pairs[:, 0].tolist(), dtype=torch.long, device=dev),
                torch.as_tensor(pairs[:, 1].tolist(), dtype=torch.long, device=dev))
    return matcher


def per_call_us(fn, calls):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls


def main():
    print("%s, torch %s, %d calls per figure" % (torch.cuda.get_device_name(0), torch.__version__, CALLS))
    d = R.load_case("e")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    as_bool = [Inst(dev(d["class_" + s]), dev(d["masks_" + s])) for s in ("n", "m", "0")]
    as_f32 = [Inst(i.pred_classes, i.pred_masks.float()) for i in as_bool]
    hip = HungarianMatcher()
    solvers = [("numpy solver", R.linear_sum_assignment)] + ([("scipy", scipy_lsa)] if scipy_lsa else [])
    want = [tuple(p) for p in d["pairs"].tolist()]
    assert list(zip(*(s.tolist() for s in hip(*as_bool)))) == want
    print("1. one call, case e (192x640, N = 20 / 20 / 8, %d pairs)" % len(want))
    t_bool, t_f32 = per_call_us(lambda: hip(*as_bool), CALLS), per_call_us(lambda: hip(*as_f32), CALLS)
    print("   mal_amd.matcher (bool masks)      %8.1f us" % t_bool)
    print("   mal_amd.matcher (float32 masks)   %8.1f us" % t_f32)
    for name, lsa in solvers:
        up = upstream_shaped(lsa)
        assert sorted(zip(*(s.tolist() for s in up(*as_f32)))) == sorted(want)
        print("   upstream-shaped, %-16s %8.1f us" % (name, per_call_us(lambda: up(*as_f32), CALLS)))

    B, H, W, n_inst = 12, 192, 640, 3
    rng = np.random.default_rng(3)
    frames, targets = [], []
    for b in range(B):
        ell = np.stack([rng.integers(40, 150, n_inst), rng.integers(60, 580, n_inst), rng.integers(10, 30, n_inst),
                        rng.integers(12, 60, n_inst)], 1)
        shift = np.concatenate([rng.integers(-3, 4, (n_inst, 1)), rng.integers(-8, 9, (n_inst, 1)), np.zeros((n_inst, 2), np.int64)], 1)
        cls = dev(rng.integers(0, 5, n_inst))
        order = rng.permutation(n_inst)
        targets.append(Inst(cls, dev(R.ellipse_masks(ell, H, W))))
        frames.append((Inst(cls[dev(order)], dev(R.ellipse_masks((ell - shift)[order], H, W))),
                       Inst(cls, dev(R.ellipse_masks(ell + shift, H, W)))))
    color = {f: torch.rand(B, 3, H, W, device=DEV) for f in (-1, 0, 1)}
    state = {}

    def ins_model(images):
        if images.shape[0] == B:
            state["b"] = 0
            return [{"instances": t} for t in targets]
        b = state["b"]
        state["b"] += 1
        return [{"instances": frames[b][0]}, {"instances": frames[b][1]}]

    def synthesis(matcher):
        outputs = {("color", -1, 0): color[-1], ("color", 1, 0): color[1]}
        assert dyn_utils.image_synthesis({("color", 0, 0): color[0]}, outputs, 0, 0.5, ins_model, matcher)
        return outputs[("syn", -1, 0)]

    print("2. dyn_utils.image_synthesis, eager, B=%d %dx%d, %d instances per sample (forward)" % (B, H, W, n_inst))
    ref = synthesis(hip).clone()
    print("   mal_amd.matcher                   %8.1f us" % per_call_us(lambda: synthesis(hip), CALLS))
    for name, lsa in solvers:
        up = upstream_shaped(lsa)
        same = torch.equal(synthesis(up), ref)
        print("   upstream-shaped, %-16s %8.1f us   (same images: %s)" % (name, per_call_us(lambda: synthesis(up), CALLS), same))
    every = torch.arange(n_inst, device=DEV)
    t0 = per_call_us(lambda: synthesis(lambda *a: (every, every)), CALLS)
    print("   identity stand-in (no matching)   %8.1f us" % t0)


if __name__ == "__main__":
    t = time.perf_counter()
    main()
    print("(%.1f s)" % (time.perf_counter() - t))
