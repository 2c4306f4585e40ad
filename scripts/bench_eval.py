"""Validation-metrics timing (mal_amd.evaluate): the device path against upstream's host path.

    python scripts/bench_eval.py [--kitti 697] [--cityscapes 1525] [--host-kitti 697] [--host-cityscapes 40]
    python scripts/bench_eval.py --kernels-only      # the device path only (for a rocprofv3 --kernel-trace --stats run)

Synthetic data (no dataset ships with the repository): KITTI Eigen-shaped sparse ground truth at the raw recording days'
image sizes with ~4 % LiDAR-like density (tests/eval_oracle.kitti_sparse_gt, float64 as gt_depths.npz holds it), and
dense 1024x2048 float32 CityScapes ground truth (8 distinct seeded images cycled over the split); student and teacher
disparities at 192x640 (KITTI) and 192x512 (CityScapes), 24 distinct seeded maps cycled.

Device: DepthEvaluator.accumulate for student and teacher plus the two means, timed with device events after a warm-up,
fed as the validation loop makes them (batches of 12) and as one call per network.  Host: Trainer.val's per-image loop
(trainer.py:975-1051) in numpy with the oracle's two-pass resize standing in for cv2.resize, on the CPUs this process may
use; timed over --host-* images and scaled to the split (stated in the output).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import eval_oracle as EO  # noqa: E402

HBM_TBS = 8.0  # MI355X HBM3E peak


def cycled(maps, n, dev):
    d = torch.from_numpy(maps).to(dev)
    return torch.cat([d] * (n // len(maps) + 1))[:n].contiguous()


def device_pass(ev, disp, mono, batch, max_depth=100.0):
    ev.reset()
    n = disp.shape[0]
    for s in range(0, n, batch):
        ev.accumulate(disp[s:s + batch], s, "student")
        ev.accumulate(mono[s:s + batch], s, "mono", 1e-3, max_depth)
    from mal_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    for which in ("student", "mono"):
        out = torch.empty(7, dtype=torch.float64, device=disp.device)
        _lib.check(lib.mal_eval_mean(ev._out[which].data_ptr(), ev.n_images, out.data_ptr(), st), "mal_eval_mean")


def time_device(ev, disp, mono, batch, reps):
    device_pass(ev, disp, mono, batch)  # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        device_pass(ev, disp, mono, batch)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def algorithmic_bytes(ev, disp):
    """bytes a perfect implementation moves per network: the disparity maps once, per packed slot the index (sparse), the
    ground truth once, and the prediction written once and read for three select passes and the final pass"""
    slots = int(ev.offsets[-1])
    sparse = int(ev.idx.numel()) if ev.split != "cityscapes" else 0
    gt = slots * ev.gt.element_size()
    return disp.numel() * 4 + sparse * 4 + gt + slots * 4 * 5


def host_path(gts, disp_np, mono_np, split, k, max_depth=100.0):
    """Trainer.val's per-image loop for k images (student + teacher), seconds"""
    sd = EO.disp_to_depth(disp_np[:, 0], 1e-3, 80)[0]
    md = EO.disp_to_depth(mono_np[:, 0], 1e-3, max_depth)[0]
    t0 = time.perf_counter()
    for i in range(k):
        EO.evaluate_image(gts[i], sd[i % len(sd)], split, True, 1.0, pointwise=False)
        EO.evaluate_image(gts[i], md[i % len(md)], split, True, None, pointwise=False)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kitti", type=int, default=697)
    ap.add_argument("--cityscapes", type=int, default=1525)
    ap.add_argument("--host-kitti", type=int, default=697)
    ap.add_argument("--host-cityscapes", type=int, default=40)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mal_amd import build
    build.build(verbose=False)
    from mal_amd.evaluate import DepthEvaluator
    dev = torch.device("cuda:0")
    lines, rec = [], {"threads": torch.get_num_threads(), "cpus_usable": len(os.sched_getaffinity(0))}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sets = [("eigen", a.kitti, (192, 640))]
    if a.cityscapes:
        sets.append(("cityscapes", a.cityscapes, (192, 512)))
    for split, n, (h, w) in sets:
        t0 = time.perf_counter()
        if split == "eigen":
            gts = EO.kitti_sparse_gt(2024, n)
        else:
            distinct = EO.cityscapes_gt(2025, 8)
            gts = [distinct[i % 8] for i in range(n)]
        disp_np, mono_np = EO.disparities(11, 24, h, w), EO.disparities(12, 24, h, w)
        t1 = time.perf_counter()
        ev = DepthEvaluator(gts, split, dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        disp, mono = cycled(disp_np, n, dev), cycled(mono_np, n, dev)
        slots = int(ev.offsets[-1])
        say("%s: %d images, %d valid points (%.0f per image), %d packed slots, gt %s; evaluator construction %.2f s"
            % (split, n, int(ev.counts.sum()), ev.counts.mean(), slots, ev.gt.dtype, t2 - t1))
        r = rec[split] = {"images": n, "points": int(ev.counts.sum()), "slots": slots, "construct_s": t2 - t1,
                          "generate_s": t1 - t0}
        if a.kernels_only:
            for _ in range(3):
                device_pass(ev, disp, mono, 12)
            torch.cuda.synchronize()
            del ev, disp, mono, gts
            torch.cuda.empty_cache()
            continue
        for batch, label in ((12, "batches of 12"), (n, "one call per network")):
            med, best = time_device(ev, disp, mono, batch, a.reps)
            r["device_ms_" + ("b12" if batch == 12 else "one_call")] = med
            say("  device, student + teacher + means, %s: median %.3f ms, best %.3f ms (%d reps after a warm-up)"
                % (label, med, best, a.reps))
        byt = 2 * algorithmic_bytes(ev, disp)
        r["algorithmic_bytes"] = byt
        r["hbm_roofline_ms"] = byt / (HBM_TBS * 1e12) * 1e3
        say("  algorithmic bytes (both networks) %.1f MB -> %.3f ms at %.0f TB/s; one-call time is %.0f %% of that roofline"
            % (byt / 1e6, r["hbm_roofline_ms"], HBM_TBS, 100 * r["hbm_roofline_ms"] / r["device_ms_one_call"]))
        k = min(n, a.host_kitti if split == "eigen" else a.host_cityscapes)
        if k:
            secs = host_path(gts, disp_np, mono_np, split, k)
            r["host_s_measured"], r["host_images"] = secs, k
            r["host_s_split"] = secs * n / k
            say("  host (numpy + the oracle's two-pass resize for cv2.resize, %d torch threads, %d CPUs usable), student + "
                "teacher: %.2f s for %d images -> %.2f s for the split%s"
                % (rec["threads"], rec["cpus_usable"], secs, k, r["host_s_split"], "" if k == n else " (scaled)"))
        del ev, disp, mono, gts
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
