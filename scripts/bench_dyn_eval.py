"""DynamicDepth's validation metrics (mal_amd.dyn_eval) against the same rule in torch's operators on the device.

    python scripts/bench_dyn_eval.py                 # prints; profiles/dyn_eval_bench.txt is a copy of the output
    python scripts/bench_dyn_eval.py --kernels-only  # the device route alone, eagerly (for a kernel-trace run)

One call = one validation batch of B = 12 at disparity 192x512: the student's and the teacher's accumulate.
  (a) eigen       KITTI-sized sparse float64 ground truth at ~4 % density (tests/eval_oracle.kitti_sparse_gt)
  (b) cityscapes  dense float32 1024x2048 ground truth, the 512x1664 window (tests/eval_oracle.cityscapes_gt, 8 distinct images)
Routes:
  device         DynamicDepthEvaluator.accumulate x 2 (four launches)
  torch hoisted  trainer.py:1158-1257 image by image in torch's operators, with every host read taken out so that it can be
                 captured: the boolean-mask gathers become gathers by precomputed indices, the object region a weight
  torch as is    the same lines with upstream's host reads left in (boolean-mask gathers, ``doj_mask.sum() > 0``, one
                 ``.cpu()`` per metric): cannot be captured, timed eagerly between two events
Measured as scripts/bench_dyn_loss.py measures: ONE captured graph of back-to-back calls, call i on argument block i mod 8
(cold; a block is its own batch of the split with its own disparities and masks) or on one block (warm), replayed between two
events outside the graph; median and spread of 7 rounds, routes alternating.  The device route counts as faster only if the gap
exceeds the spread of the rounds.  The byte floor: disparities and masks once, per point the index (sparse), the ground truth
and the prediction written once, against 8 TB/s.
"""
from __future__ import annotations

import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dyn_eval_restated as R  # noqa: E402
from tests import eval_oracle as EO  # noqa: E402

DEV = torch.device("cuda:0")
B, H, W = 12, 192, 512
REPLAYS, ROUNDS, BLOCKS = 5, 7, 8
MIN_DEPTH, MAX_DEPTH = 0.1, 100.0
HBM_TBS = 8.0


def make_split(split):
    n = B * BLOCKS
    if split == "eigen":
        gts = EO.kitti_sparse_gt(2031, n)
    else:
        distinct = EO.cityscapes_gt(2032, 8)
        gts = [distinct[i % 8] for i in range(n)]
    g = torch.Generator().manual_seed(77)
    disp = torch.rand(n, 1, H, W, generator=g).to(DEV)
    mono = torch.rand(n, 1, H, W, generator=g).to(DEV)
    mask = (F.avg_pool2d(torch.rand(n, 1, H, W, generator=g), 31, 1, 15) > 0.52).float().to(DEV)   # blobs, ~a tenth of the image
    # what the torch routes need per image, on the device
    imgs = []
    for i, gt in enumerate(gts):
        g_c, m, size, (y0, x0) = R.valid_points(gt, split)
        idx = torch.from_numpy(np.flatnonzero(m)).to(DEV)
        imgs.append({"gt": torch.from_numpy(np.ascontiguousarray(g_c)).to(DEV), "mask": torch.from_numpy(m).to(DEV), "idx": idx,
                     "size": list(size), "window": split == "cityscapes"})
        imgs[-1]["gt_pts"] = imgs[-1]["gt"].reshape(-1)[idx]
    return gts, disp, mono, mask, imgs


def resized(d, im):
    depth = 1 / (1 / MAX_DEPTH + (1 / MIN_DEPTH - 1 / MAX_DEPTH) * d)
    p = torch.clamp(F.interpolate(depth, im["size"], mode="bilinear", align_corners=False), 1e-3, 80).squeeze()
    return p[256:, 192:1856] if im["window"] else p


def region_of(mask, im):
    dm = F.interpolate(mask, im["size"])[0][0]
    return dm[256:, 192:1856] if im["window"] else dm


def weighted_errors(gt, pred, w):
    """compute_depth_errors over the points with weight 1: means as sums over the weight (no data-dependent shape)"""
    n = w.sum()
    thresh = torch.max((gt / pred), (pred / gt))
    a = [((thresh < t).float() * w).sum() / n for t in R.THRESHOLDS]
    d = gt - pred
    return torch.stack([(d.abs() / gt * w).sum() / n, (d ** 2 / gt * w).sum() / n, torch.sqrt((d ** 2 * w).sum() / n),
                        torch.sqrt(((torch.log(gt) - torch.log(pred)) ** 2 * w).sum() / n)] + [x.double() for x in a])


def torch_hoisted(blk):
    out = []
    for i in blk["images"]:
        im = blk["imgs"][i]
        reg = region_of(blk["mask"][i:i + 1], im).reshape(-1)[im["idx"]].bool().to(im["gt_pts"].dtype)
        for d in (blk["disp"], blk["mono"]):
            p = resized(d[i:i + 1], im).reshape(-1)[im["idx"]]
            p = p * (torch.median(im["gt_pts"]) / torch.median(p)).float()
            p = torch.clamp(p, min=1e-3, max=80)
            out.append(torch.stack([x.double() for x in R.compute_depth_errors(im["gt_pts"], p)]))
            out.append(weighted_errors(im["gt_pts"], p, reg))
    return torch.stack(out)


def torch_as_is(blk):
    """upstream's lines with their host reads"""
    losses = {}
    for i in blk["images"]:
        im = blk["imgs"][i]
        gt, mask = im["gt"], im["mask"]
        preds = []
        for d in (blk["disp"], blk["mono"]):
            p = resized(d[i:i + 1], im).clone()
            p *= torch.median(gt[mask]) / torch.median(p[mask])
            preds.append(torch.clamp(p, min=1e-3, max=80))
        doj = mask * region_of(blk["mask"][i:i + 1], im).bool()
        losses["dojpxs"] = losses.get("dojpxs", 0) + doj.sum()
        losses["allpxs"] = losses.get("allpxs", 0) + mask.sum()
        errs = [R.compute_depth_errors(gt[m], p[m]) for p in preds for m in (mask, doj)]
        for e in errs:
            for k, m in enumerate(R.METRICS):
                if doj.sum() > 0:
                    losses[m] = losses.get(m, 0.0) + np.array(e[k].cpu())
    return losses


def device_route(blk):
    ev = blk["ev"]
    ev.accumulate(blk["disp"][blk["first"]:blk["first"] + B], blk["mask"][blk["first"]:blk["first"] + B], blk["first"], "student",
                  MIN_DEPTH, MAX_DEPTH)
    ev.accumulate(blk["mono"][blk["first"]:blk["first"] + B], blk["mask"][blk["first"]:blk["first"] + B], blk["first"], "mono",
                  MIN_DEPTH, MAX_DEPTH)


ROUTES = {"device": device_route, "torch hoisted": torch_hoisted}


def capture(route, blocks, per_graph):
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ROUTES[route](blocks[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        for i in range(per_graph):
            ROUTES[route](blocks[i % len(blocks)])
    g.replay()
    torch.cuda.synchronize()
    return g


def replay_us(g, per_graph):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(REPLAYS):
        g.replay()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / (REPLAYS * per_graph)


def eager_us(fn, blocks):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for b in blocks:
        fn(b)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / len(blocks)


def agreement(blk):
    """the routes compute the same thing on the first block"""
    ev = blk["ev"]
    device_route(blk)
    t = torch_hoisted(blk).cpu().numpy().reshape(B, 2, 2, 7)   # image, network, region, metric
    for w, who in enumerate(("student", "mono")):
        rows = ev.rows(who)[blk["first"]:blk["first"] + B].cpu().numpy()
        for reg in (0, 1):
            got, want = rows[:, 7 * reg:7 * reg + 7], t[:, w, reg]
            live = rows[:, 16] > 0 if reg else np.ones(B, bool)
            d = np.abs(got[live] - want[live]) / np.abs(want[live])
            # each route resizes with its own roundings and takes its own near-threshold comparisons
            assert d[:, :4].max() <= 1e-3 and np.abs(got[live, 4:] - want[live, 4:]).max() <= 5e-3, (who, reg, d.max(0))
    return float(rows[:, 15].mean()), float(rows[:, 16].mean())


def main():
    from mal_amd import build
    build.build(verbose=False)
    from mal_amd.dyn_eval import DynamicDepthEvaluator
    kernels_only = "--kernels-only" in sys.argv
    print("%s, torch %s; graphs of back-to-back calls, %d replays per figure, %d rounds, routes alternating"
          % (torch.cuda.get_device_name(0), torch.__version__, REPLAYS, ROUNDS))
    print("one call = the student's and the teacher's accumulate of one batch: B=%d, disparity %dx%d" % (B, H, W))
    for split in ("eigen", "cityscapes"):
        gts, disp, mono, mask, imgs = make_split(split)
        ev = DynamicDepthEvaluator(gts, split, DEV)
        blocks = [{"ev": ev, "first": k * B, "images": range(k * B, k * B + B), "disp": disp, "mono": mono, "mask": mask, "imgs": imgs}
                  for k in range(BLOCKS)]
        if kernels_only:
            for _ in range(3):
                for b in blocks:
                    device_route(b)
            torch.cuda.synchronize()
            continue
        n_all, n_doj = agreement(blocks[0])
        slots = int(ev.offsets[B] - ev.offsets[0])
        pts = int(ev.counts[:B].sum())
        per_pt = (4 if split == "eigen" else 0) + ev.gt.element_size() + 4
        floor = 2 * (B * H * W * 4 * 2 + (pts if split == "eigen" else slots) * per_pt)
        print("%s: ground truth %s, %.0f valid points per image (%.0f in the object region), %d packed slots per batch"
              % (split, ev.gt.dtype, n_all, n_doj, slots))
        result = {}
        for regime, use in (("cold (8 argument blocks in rotation)", blocks), ("warm (one argument block)", blocks[:1])):
            per = {"device": 16, "torch hoisted": 8}
            graphs = {name: capture(name, use, per[name]) for name in ROUTES}
            times = {name: [] for name in ROUTES}
            times["torch as is"] = []
            torch_as_is(use[0])
            for _ in range(ROUNDS):
                for name in ROUTES:
                    times[name].append(replay_us(graphs[name], per[name]))
                times["torch as is"].append(eager_us(torch_as_is, use))
            med = {name: statistics.median(t) for name, t in times.items()}
            print(" " + regime)
            for name, t in times.items():
                print("   %-14s %10.1f us   (%.1f .. %.1f)%s" % (name, med[name], min(t), max(t), "   eager, with its host reads" if name == "torch as is" else ""))
            print("   device / torch hoisted = %.4f, device / torch as is = %.4f" % (med["device"] / med["torch hoisted"], med["device"] / med["torch as is"]))
            result[regime] = (med, times)
            del graphs
        med, times = result["cold (8 argument blocks in rotation)"]
        spread = max(max(times[k]) - min(times[k]) for k in ("device", "torch hoisted"))
        verdict = "beats" if med["torch hoisted"] - med["device"] > spread else "does NOT beat"
        print(" cold: device %s the hoisted torch route by more than the measured spread (%.1f us apart, spread %.1f us)"
              % (verdict, med["torch hoisted"] - med["device"], spread))
        print(" byte floor per call %.2f MB -> %.2f us at %.0f TB/s; the cold device call is %.1f x that"
              % (floor / 1e6, floor / (HBM_TBS * 1e12) * 1e6, HBM_TBS, med["device"] / (floor / (HBM_TBS * 1e12) * 1e6)))
        del ev, blocks, disp, mono, mask, imgs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    t = time.perf_counter()
    main()
    print("(%.1f s)" % (time.perf_counter() - t))
