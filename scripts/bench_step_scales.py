"""Cold-regime ms/step of the headline step -- B=12 192x640, --temporal --distil, the real producer -- with one scale
(sclm = 0, what bench.py times) and with upstream's --scales 0 1 2 3 (sclm = 3), in ONE run, alternating.

    python scripts/bench_step_scales.py [--steps 300] [--rounds 7] [--rotate 6]

Both use bench.py's pieces unchanged: its synthetic batch, its Step (dyn_utils.image_synthesis with the stand-in
segmenter, three instances per sample, in-kernel tie-break noise) and its six-batch rotation, each batch with its own
workspace slot and HIP graph, so that no replay finds the previous one's working set in the Infinity Cache.  For sclm = 3
the lower scales' disparities are pooled copies of scale 0 (the shipped decoder emits scale 0 only).  Prints one JSON
line: the median ms/step of each over the rounds, their difference, and the algorithmic bytes of the extra scales' warp
kernel (warp_scales_kernel) with its time at the 8 TB/s HBM peak.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402

SCLM = 3


class ScalesStep(bench.Step):
    """bench.Step's --temporal --distil step with ("disp", s) of both networks for s = 1..sclm"""

    def __init__(self, dev, seed, sclm):
        super().__init__(dev, seed, "step")
        self.sclm = sclm
        self.lp.opt.sclm = sclm
        pool = torch.nn.functional.avg_pool2d
        self.low = {name: {s: pool(self.leaves[name].detach(), 2 ** s).clone().requires_grad_(True) for s in range(1, sclm + 1)}
                    for name in ("disp_teacher", "disp_student")}

    def __call__(self):
        if not self.sclm:
            return super().__call__()
        lv = self.leaves
        for t in lv.values():
            t.grad = None
        mono_outputs = {("disp", 0): lv["disp_teacher"]}
        for f, s in ((-1, "m1"), (1, "p1")):
            mono_outputs[("axisangle", 0, f)] = lv["axisangle_" + s]
            mono_outputs[("translation", 0, f)] = lv["translation_" + s]
        outputs = {("disp", 0): lv["disp_student"], "consistency_mask": self.cmask, "augmentation_mask": self.aug,
                   "lowest_cost": self.lowest}
        for s in range(1, self.sclm + 1):
            mono_outputs[("disp", s)] = self.low["disp_teacher"][s]
            outputs[("disp", s)] = self.low["disp_student"][s]
        losses, _, _ = self.step_mod.loss_step(self.lp.opt, self.inputs, mono_outputs, outputs, want_maps=False,
                                               image_synthesis=self.synth)
        losses["loss"].backward(gradient=self.one)
        self.losses = losses
        return losses["loss"]


class ScalesRotation(bench.Rotation):
    """bench.Rotation over ScalesStep batches"""

    def __init__(self, dev, seed, sclm, R, slot_base):
        from mal_amd import step as step_mod
        self.step_mod, self.R, self.slot_base, self.i = step_mod, R, slot_base, 0
        self.steps = [ScalesStep(dev, seed + 7919 * k, sclm) for k in range(R)]
        self.graphs, self.note = None, None
        self.capture()


def time_ms(rot, steps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        rot()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rotate", type=int, default=6)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from mal_amd import build
    build.build(verbose=False)
    rots = {s: ScalesRotation(dev, 1234, s, a.rotate, slot_base=500 + 50 * s) for s in (0, SCLM)}
    for r in rots.values():
        if r.graphs is None:
            raise SystemExit(r.note)
        time_ms(r, 3 * a.rotate)  # warm-up replays
    ms = {s: [] for s in rots}
    for _ in range(a.rounds):
        for s, r in rots.items():
            ms[s].append(time_ms(r, a.steps))
    med = {s: statistics.median(v) for s, v in ms.items()}
    B, H, W = bench.B, bench.H, bench.W
    # per pixel and extra scale of the teacher: 24 B of warped images written + ~24 B of texels gathered (two frames, the
    # taps of neighbouring pixels shared through the caches); the low-resolution disparity adds < 1 B
    kernel_bytes = SCLM * B * H * W * (24 + 24)
    print(json.dumps({"shape": [B, H, W], "config": "--temporal --distil, real producer, %d-batch rotation, graphs" % a.rotate,
                      "ms_per_step_sclm0": med[0], "ms_per_step_sclm3": med[SCLM], "added_ms": med[SCLM] - med[0],
                      "rounds_sclm0": ms[0], "rounds_sclm3": ms[SCLM],
                      "warp_scales_kernel_bytes": kernel_bytes,
                      "warp_scales_kernel_us_at_8TBps": kernel_bytes / 8e12 * 1e6}))


if __name__ == "__main__":
    main()
