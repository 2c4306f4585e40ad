#!/usr/bin/env python
"""bench.py -- MAL photometric-reprojection + motion-aware-loss path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    (N>1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...)

One "step" = one pass of the hot path over one synthetic KITTI-shaped batch per GPU
(B=12, 192x640, BASELINE.json configs[1]): process_batch's loss half --
teacher pass (warp + SSIM/L1 + min + automask, forward+backward to disparity and poses),
ensemble pass (no grad), student pass (+ consistency + distillation), the two smoothness
terms, pose composition and the full backward to the four leaves
(manydepth/trainer.py:573-642).  Inputs are resident in HBM before the timed region.
The path shards by batch with no data-path collective (each DDP rank
normalises over its own batch); ranks are replicas over disjoint batches -> weak scaling.

At N>1 (one process per GPU over RCCL; `--gpus N` without WORLD_SIZE spawns the N ranks itself through
torch.distributed.run BEFORE anything touches the GPU) every step ends with the data-parallel exchange of the
trainer -- ONE all-reduce of the flat 165 MB fp32 gradient bucket of RepDepth (mal_amd/dp.py; manydepth/trainer.py:
309-311,469) -- timed inside the step and reported as its own `breakdown_ms` entry.

Prints ONE JSON line (rank 0) with the contract fields.  A plain run does nothing else: it sets up, warms up, times the
--steps steps and prints the line.  `--full` adds every side measurement, each in extra work after the timed steps:
  roofline:     the teacher-pass fused kernel, timed live with HIP events on its stream (--mode step only)
  cpu_baseline: the CPU oracle (PyTorch-CPU restatement == the reference's path) on the host
  train_step:   the WHOLE training step of the harness (networks through MIOpen + this loss path + all-reduce + Adam):
                images/s and per-stage breakdown, so that the loss-path rate in `value` is never read as training throughput.
  and the warm regime, the eager step, the stage breakdown, the overlapped exchange (N>1) and the channels_last variant.
`--dump-outputs DIR` writes what the last timed step handed its caller (the loss dictionary and the leaves' gradients) as
DIR/<name>.npy; the same arguments give the timed steps the same inputs in every run.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, H, W = 12, 192, 640
ALG_BYTES_PER_PX = 96      # fused warp+SSIM+min-reproj+automask fwd+bwd, fp32, F=2
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--graph", type=int, default=1, help="1: replay the step from a HIP graph (default); 0: eager launches")
    ap.add_argument("--mode", choices=["step", "distil", "ops", "temporal", "train", "multiscale", "multiscale_ops", "dualrefine",
                                       "dualrefine_ops"], default="step",
                    help="step: --temporal --distil through mal_loss_step (BASELINE configs[1], the headline: three library "
                         "calls around the temporal-hint producer); distil: --distil only (one C call per direction); "
                         "ops: the operator-level API; "
                         "temporal: --temporal --distil through the operator-level API; train: the whole training step "
                         "of the harness (RepDepth networks + loss step + flat-bucket all-reduce + Adam, eager); "
                         "multiscale: the non-distil compute_losses with sclm=3 (four disparity scales, "
                         "manydepth/trainer.py:1248-1475) for both networks through mal_loss_multiscale (one C call per "
                         "direction); multiscale_ops: the same through the operator-level API; dualrefine: BASELINE configs[4], "
                         "DualRefine's loss loops over (scale 0, deq_iter 0..1) at B=8 (dualrefine/trainer.py:395-451,530-633) "
                         "through DualRefineLossPath.loss_step (mal_dr_loss_fwd/_bwd, one call per direction); dualrefine_ops: the same through "
                         "generate_images_pred + compute_losses (operator-level route)")
    ap.add_argument("--width", type=int, default=640, help="image width: 640 (KITTI, the headline) or 512 (CityScapes, "
                                                            "BASELINE configs[3]); the metric string follows it")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--loss-blc", action="store_true",
                    help="add the `loss_blc` block: the same step with --loss_blc (the reference's KITTI command, README.md:22; "
                         "manydepth/loss_utils.py:303-345, trainer.py:640-642): LossBalancing's weights enter the step as host "
                         "scalars that change every step and its score table needs the two loss scalars on the host, so the "
                         "steps are eager launches with one device->host read each")
    ap.add_argument("--channels-last", action="store_true",
                    help="hand the three (B,3,H,W) images over in torch.channels_last memory format: they ARE the texel images the "
                         "passes gather from, the step skips its re-layout (MAL_STEP_TEXEL_INPUTS).  The default (the headline) "
                         "keeps the reference's NCHW tensors and reports this variant in the `channels_last` side block")
    ap.add_argument("--main-temporal", action="store_true",
                    help="--mode step with --main_temporal as well (manydepth/trainer.py:1164, loss_utils.py:152-155): the student's "
                         "warped images go through the producer too (MAL_STEP_MAIN_TEMPORAL); a variant run, not the headline")
    ap.add_argument("--dr-default-scales", action="store_true",
                    help="--mode dualrefine / dualrefine_ops with upstream's default scale list [0,1,2,3] (dualrefine/options.py:65-69: "
                         "scale 0 and 2 with both deq iterations, scale 1 skipped, scale 3 iteration 0) instead of [0]; a variant run")
    ap.add_argument("--dr-pose-update", action="store_true",
                    help="--mode dualrefine / dualrefine_ops with the pose updates on (dualrefine/trainer.py:335-343,457-480,699-767): "
                         "the pose-update losses ride on the one-call step as one more marching pass (MAL_DR_POSE_UPDATE); a variant run")
    ap.add_argument("--ms-temporal", action="store_true",
                    help="--mode multiscale with --temporal (trainer.py:1161-1162,1279-1283): the producer once per scale between "
                         "mal_loss_multiscale_warp and _fwd; a variant run")
    ap.add_argument("--value", choices=["auto", "loss", "train"], default="auto",
                    help="what the line's `value` is: loss (= auto, at every N) = the loss path, with the whole training step in the "
                         "`train_step` block of the same line and `scaling_quantity` naming it as the field the DP-scaling ratio "
                         "is taken from; train = the line's value / ms_per_step ARE the whole training step's")
    ap.add_argument("--rotate", type=int, default=6,
                    help="the timed steps rotate over this many distinct synthetic batches, each with its own inputs, leaves and "
                         "step workspace (>= 6 x ~190 MB: nothing a step reads is left in the 256 MiB Infinity Cache by the "
                         "previous pass over the same batch -- the COLD regime, what a training step sees after 45 ms of "
                         "convolution traffic); 1 = replay one batch (the warm regime of rounds 1-4)")
    ap.add_argument("--regime", choices=["both", "cold", "warm"], default="both",
                    help="both (default): the line's value / roofline are the cold regime's, the warm figures sit beside them; "
                         "cold / warm: measure only that regime (rocprofv3 runs: per-kernel averages of one regime)")
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=INT",
                    help="mal_set_option before the run (kernel experiments, e.g. march_rows=16)")
    ap.add_argument("--cpu-steps", type=int, default=10, help="timed CPU-oracle steps (median), after 3 warm-ups")
    ap.add_argument("--train-steps", type=int, default=20,
                    help="steps of the whole training step timed for the `train_step` block after 3 warm-ups (0 = leave it out)")
    ap.add_argument("--full", action="store_true",
                    help="every side measurement after the timed steps (warm regime, eager step, breakdown, roofline, "
                         "channels_last, train_step, cpu_baseline); a plain run measures the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (loss dictionary, leaf gradients) as DIR/<name>.npy")
    return ap.parse_args()


N_GRAD_PARAMS = 41_247_150  # trainable fp32 parameters of RepDepth (tests/test_networks.py): 165 MB


def visible_gpus():
    """GPUs of this node WITHOUT touching HIP (the launcher process must stay free of the runtime): the KFD topology lists
    every node, GPUs are the ones with SIMDs; ROCR/HIP_VISIBLE_DEVICES narrow it.  None if the topology is unreadable."""
    if not os.path.isdir("/sys/class/kfd"):
        return 0  # no amdgpu compute driver on this machine at all
    try:
        base = "/sys/class/kfd/kfd/topology/nodes"
        n = 0
        for node in os.listdir(base):
            with open(os.path.join(base, node, "properties")) as fh:
                props = dict(l.split()[:2] for l in fh if len(l.split()) >= 2)
            if int(props.get("simd_count", "0")) > 0:
                n += 1
    except Exception:
        return None
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([x for x in v.split(",") if x.strip() != ""]))
    return n


def spawn_ranks(args):
    """`bench.py --gpus N` on its own: start the N ranks (one process per GPU) as children through
    torch.distributed.run and relay rank 0's JSON line.  This process makes no HIP call at all (the GPUs are counted from
    the KFD topology in sysfs; a process that has initialised the GPU must not exec or be re-used as a launcher on this
    pool); a failing rank makes the whole launch exit non-zero."""
    import socket
    import subprocess
    if os.environ.get("MAL_BENCH_BACKEND", "nccl") == "nccl":
        n = visible_gpus()
        if n is not None and n < args.gpus:  # unreadable topology: let the ranks fail with their own message
            raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible" % (args.gpus, n))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


OUTPUT_BYTES_CAP = 64 << 20  # --dump-outputs: larger outputs are written as a fixed, seeded sample of their elements


def host_outputs(st):
    """what the caller of the timed path received from `st`'s last step, on the host: the tensors of its loss dictionary and,
    for a loss step, the gradients of its leaves"""
    out = {"loss." + str(k): v for k, v in st.losses.items() if torch.is_tensor(v)}
    for k, v in getattr(st, "leaves", {}).items():
        if v.grad is not None:
            out["grad." + k] = v.grad
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def write_outputs(d, arrays):
    """DIR/<name>.npy in float32 (float64 stays float64), at most OUTPUT_BYTES_CAP in all"""
    import re
    import numpy as np
    arrays = {k: np.asarray(a, dtype=np.float64 if a.dtype in (np.float64, np.int64, np.int32) else np.float32)
              for k, a in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    budget = OUTPUT_BYTES_CAP - 256 * len(arrays)  # room for the .npy headers
    rng = np.random.default_rng(0)
    os.makedirs(d, exist_ok=True)
    for k in sorted(arrays):
        a = arrays[k]
        if total > budget and a.size > 1:
            n = max(1, int(a.size * budget // total))
            a = a.reshape(-1)[np.sort(rng.choice(a.size, n, replace=False))]
        np.save(os.path.join(d, re.sub(r"[^A-Za-z0-9_.-]+", "_", k) + ".npy"), a)


class TrainStep:
    """--mode train: mal_amd.harness.TrainHarness on a synthetic batch (next row N1; not the headline metric)."""

    def __init__(self, dev, seed):
        import random
        from mal_amd import config, harness
        config.noise_source = "cuda"
        random.seed(seed)
        torch.manual_seed(seed)
        # BASELINE configs[1] as written: --temporal --distil; the temporal hint's two external models (Mask2Former, the
        # Hungarian matcher: out of scope) are the same stand-ins the headline step uses, three instances per sample
        from mal_amd import dyn_utils
        from mal_amd.synthetic import instance_stub
        self.opt = harness.default_options(batch_size=B, height=H, width=W, temporal=True)
        ins_model, matcher = instance_stub(B, H, W, n_inst=3, seed=seed, device=dev)
        synth = lambda inputs, outputs, scale: dyn_utils.image_synthesis(inputs, outputs, scale, 0.5, ins_model, matcher)
        self.h = harness.TrainHarness(self.opt, dev, image_synthesis=synth)
        self.inputs = harness.synthetic_inputs(self.opt, dev, seed=seed)
        self.batch_cpu = None

    def __call__(self):
        self.losses = self.h.train_step(self.inputs)
        return self.losses["loss"]

    def breakdown_ms(self, steps=5):
        """mean device time per stage over a few extra steps outside the timed region"""
        from mal_amd.harness import StageTimer
        acc = {}
        for _ in range(steps):
            t = StageTimer()
            self.h.train_step(self.inputs, t)
            for k, v in t.result_ms().items():
                acc[k] = acc.get(k, 0.0) + v / steps
        return acc


class Step:
    """Everything a step needs, resident on the device."""

    def __init__(self, dev, seed, mode="step", channels_last=False, main_temporal=False, ms_temporal=False, dr_scales=None,
                 dr_pose_update=False):
        from mal_amd import config, layers, trainer, step as step_mod
        self.mode, self.step_mod = mode, step_mod
        from mal_amd.synthetic import make_batch
        # no host randn / H2D on the step: the whole-step API draws the tie-break noise inside its first
        # kernel (Philox, keyed per rank); the operator-level modes use the device generator
        config.noise_source = "philox" if mode in ("step", "distil", "multiscale", "dualrefine") else "cuda"
        config.noise_seed = 0x4d414c5eed + seed
        config.consistency_target = False  # logging-only map (loss_utils.py:212-215)
        self.one = torch.ones((), dtype=torch.float32, device=dev)  # d(loss)/d(loss): handed to backward, no fill launch
        self.layers = layers
        from mal_amd import ops
        self.ops = ops
        self.dr_ops = mode == "dualrefine_ops"
        if self.dr_ops:
            mode = self.mode = "dualrefine"
        self.B = 8 if mode == "dualrefine" else B  # BASELINE configs[4] is quoted at B=8
        b = make_batch(self.B, H, W, seed=seed)
        mv = lambda t: t.to(dev).contiguous()
        self.inputs = {("color", 0, 0): mv(b["color0"]), ("color", -1, 0): mv(b["color_m1"]),
                       ("color", 1, 0): mv(b["color_p1"]), ("K", 0): mv(b["K"]), ("inv_K", 0): mv(b["inv_K"])}
        if channels_last:  # same values, the texel layout: (B,3,H,W) with strides (3HW, 1, 3W, 3)
            for f in (0, -1, 1):
                self.inputs[("color", f, 0)] = self.inputs[("color", f, 0)].contiguous(memory_format=torch.channels_last)
        self.leaves = {k: mv(b[k]).requires_grad_(True) for k in
                       ("disp_teacher", "disp_student", "axisangle_m1", "translation_m1", "axisangle_p1",
                        "translation_p1")}
        self.cmask, self.aug, self.lowest = mv(b["consistency_mask"]), mv(b["augmentation_mask"]), mv(b["lowest_cost"])
        self.synth = None
        if mode in ("temporal", "step"):
            # --temporal --distil: dyn_utils.image_synthesis itself (N2: the patch shifts in HIP) with stand-ins for its
            # two external models (Mask2Former, Hungarian matcher: out of scope), three matched instances per sample
            from mal_amd import dyn_utils
            from mal_amd.synthetic import instance_stub
            ins_model, matcher = instance_stub(B, H, W, n_inst=3, seed=seed, device=dev)
            synth = lambda inputs, outputs, scale: dyn_utils.image_synthesis(inputs, outputs, scale, 0.5, ins_model, matcher)
            self.synth = synth
            self.lp = trainer.LossPath(trainer.default_options(height=H, width=W, batch_size=B, temporal=True,
                                                               main_temporal=bool(main_temporal and mode == "step")), fuse=True,
                                       image_synthesis=synth)
        elif mode == "dualrefine":
            from mal_amd import dualrefine
            self.dr_scales = list(dr_scales or [0])
            self.dr_pose_update = bool(dr_pose_update)
            self.lp = dualrefine.DualRefineLossPath(dualrefine.default_options(height=H, width=W, batch_size=self.B, n_losses=1,
                                                                               scales=self.dr_scales,
                                                                               disable_pose_updates=not dr_pose_update), fuse=True)
            self.cmask4 = self.cmask.unsqueeze(1)
            for sc in self.dr_scales:  # lower scales: pooled copies (the DEQ decoder is not part of this package)
                if sc in (0, 1):
                    continue
                self.inputs[("color", 0, sc)] = torch.nn.functional.avg_pool2d(self.inputs[("color", 0, 0)], 2 ** sc)
                for it, name in ((0, "disp_teacher"), (1, "disp_student")):
                    if sc == 3 and it > 0:
                        continue
                    self.leaves["disp_s%d_it%d" % (sc, it)] = torch.nn.functional.avg_pool2d(mv(b[name]), 2 ** sc).clone().requires_grad_(True)
        elif mode in ("multiscale", "multiscale_ops"):
            # --scales 0..3 semantics (sclm=3): per-scale disparities upsampled to full resolution, loss
            # / 2**scale, total / (sclm+1); the shipped decoder only feeds scale 0, so the lower scales are pooled copies
            self.lp = trainer.LossPath(trainer.default_options(height=H, width=W, batch_size=B, sclm=3, distil=False,
                                                               temporal=bool(ms_temporal and mode == "multiscale")), fuse=True)
            if ms_temporal and mode == "multiscale":
                from mal_amd import dyn_utils
                from mal_amd.synthetic import instance_stub
                ins_model, matcher = instance_stub(B, H, W, n_inst=3, seed=seed, device=dev)
                self.synth = lambda inputs, outputs, scale: dyn_utils.image_synthesis(inputs, outputs, scale, 0.5, ins_model, matcher)
            for sc in (1, 2, 3):
                k = 2 ** sc
                self.inputs[("color", 0, sc)] = torch.nn.functional.avg_pool2d(self.inputs[("color", 0, 0)], k)
                for name in ("disp_teacher", "disp_student"):
                    self.leaves["%s_s%d" % (name, sc)] = torch.nn.functional.avg_pool2d(mv(b[name]), k).clone().requires_grad_(True)
        else:
            self.lp = trainer.LossPath(trainer.default_options(height=H, width=W, batch_size=B), fuse=True)
        self.batch_cpu = b

    def __call__(self):
        L, lv = self.layers, self.leaves
        for t in lv.values():
            t.grad = None
        if self.mode in ("step", "distil"):  # the whole-step API (texel packing redone every step: a real step sees new images)
            mono_outputs = {("disp", 0): lv["disp_teacher"]}
            for f, s in ((-1, "m1"), (1, "p1")):
                mono_outputs[("axisangle", 0, f)] = lv["axisangle_" + s]
                mono_outputs[("translation", 0, f)] = lv["translation_" + s]
            outputs = {("disp", 0): lv["disp_student"], "consistency_mask": self.cmask,
                       "augmentation_mask": self.aug, "lowest_cost": self.lowest}
            losses, _, _ = self.step_mod.loss_step(self.lp.opt, self.inputs, mono_outputs, outputs, want_maps=False,
                                                   image_synthesis=self.synth)
            losses["loss"].backward(gradient=self.one)
            self.losses = losses
            return losses["loss"]
        if self.mode == "multiscale":  # trainer.py:573-612 with not opt.distil, both networks, four scales: one call
            mono_outputs = {("disp", 0): lv["disp_teacher"]}
            for f, s in ((-1, "m1"), (1, "p1")):
                mono_outputs[("axisangle", 0, f)] = lv["axisangle_" + s]
                mono_outputs[("translation", 0, f)] = lv["translation_" + s]
            outputs = {("disp", 0): lv["disp_student"], "consistency_mask": self.cmask, "augmentation_mask": self.aug,
                       "lowest_cost": self.lowest}
            for sc in (1, 2, 3):
                mono_outputs[("disp", sc)] = lv["disp_teacher_s%d" % sc]
                outputs[("disp", sc)] = lv["disp_student_s%d" % sc]
            losses, _ = self.step_mod.loss_step_multiscale(self.lp.opt, self.inputs, mono_outputs, outputs, want_maps=False,
                                                           image_synthesis=self.synth)
            losses["loss"].backward(gradient=self.one)
            self.losses = losses
            return losses["loss"]
        self.ops.clear_packed_sources()  # a real step sees new images: repack them every step
        T_m1 = L.transformation_from_parameters(lv["axisangle_m1"], lv["translation_m1"], True)
        T_p1 = L.transformation_from_parameters(lv["axisangle_p1"], lv["translation_p1"], False)
        if self.mode == "dualrefine":  # 4-tuple keys: ("disp", 0, deq_iter); iteration 1 refines pose -1
            outputs = {("disp", 0, 0): lv["disp_teacher"], ("disp", 0, 1): lv["disp_student"], ("cam_T_cam", 0, -1): T_m1,
                       ("cam_T_cam", 0, 1): T_p1, ("cam_T_cam", 0, -1, 1): T_m1 * 1.0, "consistency_mask": self.cmask4}
            for k, t in lv.items():
                if k.startswith("disp_s") and k[6].isdigit():  # "disp_s<scale>_it<iteration>"
                    outputs[("disp", int(k[6]), int(k[-1]))] = t
            if self.dr_ops:  # the operator-level route (two fused passes + glue: ~75 launches)
                self.lp.generate_images_pred(self.inputs, outputs)
                losses = self.lp.compute_losses(self.inputs, outputs)
                if self.dr_pose_update:  # process_batch's second dictionary, merged as upstream merges it (:337-343)
                    self.lp.pose_update_generate_images_pred(self.inputs, outputs)
                    for k, v in self.lp.compute_pose_update_losses(self.inputs, outputs).items():
                        losses[k] = losses[k] + v if k in losses else v
            else:            # mal_dr_loss_fwd/_bwd: one library call per direction
                losses = self.lp.loss_step(self.inputs, outputs)
            losses["loss"].backward(gradient=self.one)
            self.losses = losses
            return losses["loss"]
        mono_outputs = {("disp", 0): lv["disp_teacher"], ("cam_T_cam", 0, -1): T_m1, ("cam_T_cam", 0, 1): T_p1}
        outputs = {("disp", 0): lv["disp_student"], ("cam_T_cam", 0, -1): T_m1, ("cam_T_cam", 0, 1): T_p1,
                   "consistency_mask": self.cmask, "augmentation_mask": self.aug, "lowest_cost": self.lowest}
        if self.mode == "multiscale_ops":  # trainer.py:573-612 with not opt.distil: compute_losses for both nets, op by op
            for sc in (1, 2, 3):
                mono_outputs[("disp", sc)] = lv["disp_teacher_s%d" % sc]
                outputs[("disp", sc)] = lv["disp_student_s%d" % sc]
            lp = self.lp
            lp.generate_images_pred(self.inputs, mono_outputs)
            mono_losses, _ = lp.compute_losses(self.inputs, mono_outputs, is_multi=False)
            for key in list(mono_outputs.keys()):
                if isinstance(key, tuple) and key[0] in ("depth", "disp"):
                    outputs[("mono_" + key[0],) + tuple(key[1:])] = mono_outputs[key]
            lp.generate_images_pred(self.inputs, outputs, is_multi=True)
            losses, _ = lp.compute_losses(self.inputs, outputs, is_multi=True)
            total = losses["loss"] + mono_losses["loss"]
            total.backward()
            self.losses = {"mono/%s" % (k,): v for k, v in mono_losses.items()}
            self.losses.update(losses)
            self.losses["total"] = total
            return total
        _, losses, _ = self.lp.compute_batch_losses(self.inputs, mono_outputs, outputs)
        losses["loss"].backward()
        self.losses = losses
        return losses["loss"]


class Rotation:
    """`R` synthetic batches of the same shape, each with its own inputs, leaves and step workspace (mal_amd.step.
    workspace_slot); pass i runs batch i % R -- captured as one HIP graph per batch when `graph`.  With R x (inputs + leaves +
    workspace: ~190 MB at B=12 192x640) well beyond the 256 MiB Infinity Cache, no pass finds anything the previous pass over
    the same batch left on the die: every operand comes from HBM, as in a training step (manydepth/trainer.py:465-470: the
    networks' forward and backward run between two loss calls).  R = 1 is the warm regime (one batch replayed)."""

    def __init__(self, dev, seed, mode, R, slot_base=0, graph=True, **kw):
        from mal_amd import step as step_mod
        self.step_mod, self.R, self.slot_base, self.i = step_mod, R, slot_base, 0
        self.steps = [Step(dev, seed + 7919 * k, mode, **kw) for k in range(R)]
        self.graphs, self.note = None, None
        if graph:
            self.capture()

    def call(self, k):
        with self.step_mod.workspace_slot(self.slot_base + k):
            return self.steps[k]()

    def capture(self):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for k in range(self.R):
                for _ in range(3):
                    self.call(k)
        torch.cuda.current_stream().wait_stream(s)
        try:
            graphs = []
            for k in range(self.R):
                g = torch.cuda.CUDAGraph()
                # thread_local: other threads of the process (the RCCL watchdog at N>1) may touch the runtime during capture
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self.call(k)
                graphs.append(g)
            self.graphs = graphs
        except Exception as e:  # keep the measurement alive: eager launches (host-bound, slower), and say so
            self.graphs = None
            self.note = "graph capture failed (%s: %s); eager launches" % (type(e).__name__, str(e).splitlines()[0][:120])
            torch.cuda.synchronize()

    def _run(self, k):
        if self.graphs is not None:
            self.graphs[k].replay()
        else:
            self.call(k)

    def __call__(self):  # the next pass of the rotation
        k = self.i % self.R
        self.i += 1
        self._run(k)

    def eager(self):     # ... as eager launches
        k = self.i % self.R
        self.i += 1
        return self.call(k)

    def first(self):     # batch 0 again and again: the warm regime
        self._run(0)


def measured_copy_ceiling(dev, mib=1024, reps=5):
    """device-to-device copy rate of this box (read + write bytes / time): the practical HBM ceiling next to the
    8 TB/s spec the roofline fraction is quoted against (SURVEY.md 8d asks for both)."""
    n = mib * (1 << 20) // 4
    a, b = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return 2.0 * n * 4 * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9


def shader_clock_mhz(lib, dev):
    """sustained shader clock with two packed-FMA wavefronts on every SIMD (mal_clock_probe: s_memtime ticks over the
    constant 100 MHz counter), after ~1 ms of the same load"""
    out = torch.zeros(3, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(10):
        if lib.mal_clock_probe(out.data_ptr(), 400, st) != 0:
            return None
    torch.cuda.synchronize()
    t, r = int(out[0].item()), int(out[1].item())
    return 100.0 * t / r if r > 0 else None


def valu_bound(lib, dev, kernel_ms, hbm_frac, halo1=True):
    """What actually bounds the north-star kernel: its row loop priced by instruction class from the
    compiler's listing of the shipped sources (mal_amd.build.valu_report -> mal_amd/lib/valu_cost.json; per-class
    cycles measured by scripts/valu_probe.hip), times the row-loop iterations of all tasks, over the chip's SIMDs at the
    clock measured in this run = the time the vector ALUs alone need; `valu_frac` = that / the measured kernel time."""
    try:
        from mal_amd import build, _lib
        rep = build.valu_report()
        k = rep["kernels"]["teacher"]
        g = [ctypes.c_int(0) for _ in range(4)]
        flags = _lib.F_GRAD | _lib.F_AUTOMASK | _lib.F_POSE_GRAD
        _lib.check(lib.mal_march_geometry(B, H, W, flags, *[ctypes.byref(x) for x in g]), "mal_march_geometry")
        strips, segs, rows, iters = (x.value for x in g)
        tasks = B * strips * segs
        simds = torch.cuda.get_device_properties(dev).multi_processor_count * 4
        mhz = shader_clock_mhz(lib, dev)
        if not mhz or kernel_ms <= 0:
            return {"valu": {"error": "no clock / kernel time"}}
        drain = k.get("drain", {}).get("pipe_cycles")
        if halo1 and drain:  # one-row halo of the step's gradient passes: rows + 2 warped rows, then two gradient-only iterations
            iters_full, iters_drain = rows + 2, 2
        else:
            iters_full, iters_drain, drain = iters, 0, 0.0
        cycles = (k["pipe_cycles"] * iters_full + drain * iters_drain) * tasks / simds
        valu_us = cycles / mhz
        frac = valu_us / (kernel_ms * 1e3)
        return {"bound": "valu" if frac > hbm_frac else "hbm",
                "valu": {"valu_frac": frac, "valu_us": valu_us, "pipe_cycles_per_row": k["pipe_cycles"],
                         "valu_instructions_per_row": k["valu_instructions"], "classes": k["classes"],
                         "row_iterations_per_task": iters_full, "gradient_only_iterations_per_task": iters_drain,
                         "pipe_cycles_per_gradient_only_iteration": drain, "rows_per_task": rows, "tasks": tasks, "simds": simds,
                         "shader_clock_mhz": mhz,
                         "how": "(pipe_cycles_per_row x row_iterations_per_task + pipe_cycles_per_gradient_only_iteration x "
                                "gradient_only_iterations_per_task) x tasks / simds / clock; classes from the "
                                "compiler's listing of the shipped kernel (mal_amd/lib/valu_cost.json, digest %s), cycle "
                                "prices from scripts/valu_probe.hip (profiles/r02_valu_probe.txt); an upper estimate: the "
                                "first and last iterations of a task skip the gradient / statistics stages" % rep["digest"][:12]}}
    except Exception as ex:  # the line survives; the block says why it is missing
        return {"valu": {"error": "%s: %s" % (type(ex).__name__, str(ex).splitlines()[0][:200])}}


def cpu_baseline(batch, steps, temporal, seed):
    """The CPU oracle (oracle/mal_oracle.py, PyTorch-CPU ATen ops in the reference's order) on the SAME step the GPU line
    times: B=12 192x640, passes A+B+C forward+backward; with `temporal` (the headline) incl. the temporal hint -- the
    producer restated on the CPU (oracle/dyn_oracle.image_synthesis around generate_dynamic_instance, dyn_utils.py:6-170)
    driven by the same stand-in segmenter / matcher on the same instance masks, the two synthesised candidates in the
    teacher's min and the gradient through them.  SURVEY.md 8d: median of `steps` (10) runs after 3 warm-ups on the box's
    core share; one thread (the reference's OMP_NUM_THREADS=1, manydepth/trainer.py:8-10): median of 3 after 1 warm-up, to
    keep the whole bench within minutes."""
    from mal_amd.synthetic import instance_stub, to_dicts
    from oracle import mal_oracle as O
    opt = O.default_opt(height=H, width=W, batch_size=B, temporal=bool(temporal))
    synth = None
    if temporal:
        from oracle import dyn_oracle
        ins_model, matcher = instance_stub(B, H, W, n_inst=3, seed=seed, device="cpu")
        synth = lambda inputs, outputs, scale: dyn_oracle.image_synthesis(inputs, outputs, scale, 0.5, ins_model, matcher)
    # a one-GPU box's CPU share is 16 cores: more torch threads than that oversubscribe it (128 threads measured no
    # faster than 1)
    all_threads = torch.get_num_threads()
    threads = min(all_threads, 16)
    torch.set_num_threads(threads)

    def one():
        inputs, mono_outputs, outputs, leaves = to_dicts(batch, O.transformation_from_parameters)
        losses, *_ = O.mal_loss_step(opt, inputs, mono_outputs, outputs, synth=synth)
        losses["loss"].backward()

    def median_of(n_warm, n):
        for _ in range(n_warm):
            one()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            one()
            ts.append(time.perf_counter() - t0)
        return sorted(ts)[len(ts) // 2]

    dt = median_of(3, steps)
    what = ("--temporal --distil loss step (passes A+B+C fwd+bwd incl. the temporal hint's producer on the CPU, 3 matched "
            "instances per sample)") if temporal else "--distil loss step (passes A+B+C fwd+bwd)"
    out = {"value": B / dt, "unit": "images/s", "cores": threads, "kind": "port",
           "sample": "median of %d steps of the same B=12 192x640 %s after 3 warm-ups, torch CPU threads=%d"
                     % (steps, what, threads), "ms_per_step": 1e3 * dt}
    torch.set_num_threads(1)
    dt1 = median_of(1, 3)
    torch.set_num_threads(all_threads)
    out["single_thread"] = {"value": B / dt1, "unit": "images/s", "cores": 1, "sample": "median of 3 steps after 1 warm-up",
                            "ms_per_step": 1e3 * dt1}
    return out


def teacher_enqueuers(plains, slot_base=100):
    """for every --distil step object of `plains`: one forward of that batch in its own workspace (texels, identity map,
    camera block), handing back enqueue(n) = n back-to-back launches of the teacher's pass with that forward's argument
    block (mal_loss_step_teacher_replay)"""
    from mal_amd import step as step_mod
    out = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for k, plain in enumerate(plains):
            lv = plain.leaves
            mono_outputs = {("disp", 0): lv["disp_teacher"]}
            for f, s_ in ((-1, "m1"), (1, "p1")):
                mono_outputs[("axisangle", 0, f)] = lv["axisangle_" + s_]
                mono_outputs[("translation", 0, f)] = lv["translation_" + s_]
            outputs = {("disp", 0): lv["disp_student"], "consistency_mask": plain.cmask, "augmentation_mask": plain.aug,
                       "lowest_cost": plain.lowest}
            with step_mod.workspace_slot(slot_base + k):
                enqueue = step_mod.teacher_pass_replay(plain.lp.opt, plain.inputs, mono_outputs, outputs)
            enqueue(2)
            out.append(enqueue)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return out


def replayed_kernel_ms(enqueuers, launches=64, replays=10):
    """The north-star kernel alone, as a REPLAYED graph runs it, measured in this run: a graph that holds nothing but
    `launches` back-to-back launches of the teacher's pass, launch i with the argument block of batch i % len(enqueuers)
    (mal_loss_step_teacher_replay), replayed `replays` times after two warm-up replays, timed with two events OUTSIDE the
    graph.  One enqueuer = the WARM regime (every launch re-reads the ~65 MB the previous one left in the Infinity Cache);
    eight = the COLD regime (a launch reads ~77 MB of its own batch and seven other batches' 540 MB pass through the 256 MiB
    cache before that batch comes round again: every operand is fetched from HBM).  The quotient contains the gaps between
    consecutive graph nodes (an upper bound of the kernel's own duration; rocprofv3's per-dispatch average of the same
    command, profiles/, is the kernel alone)."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for i in range(launches):
            enqueuers[i % len(enqueuers)](1)
    for _ in range(2):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (launches * replays), launches * replays


def channels_last_block(dev, seed, mode, R, steps=200):
    """the same step with the three images in torch.channels_last (zero-copy texels), graph-replayed like the headline and
    in the headline's regime (rotating over R batches)"""
    rot = Rotation(dev, seed, mode, R, slot_base=200, channels_last=True)
    for _ in range(20):
        rot()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        rot()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    return {"ms_per_step": ms, "value": B / (ms * 1e-3), "unit": "images/s", "steps": steps,
            "launch": "hip-graph" if rot.graphs is not None else rot.note, "batches_rotated": R,
            "what": "the same step with inputs[('color', f, 0)] in torch.channels_last memory format: the (B,H,W,3) texel images "
                    "themselves, no re-layout in the first sweep (MAL_STEP_TEXEL_INPUTS); a loader gets there with "
                    ".contiguous(memory_format=torch.channels_last) on the host tensor (INTEGRATION.md)"}


def loss_blc_block(dev, seed, mode, steps):
    """--loss-blc: the same step with the reference's --loss_blc (README.md:22): total = bs * (w0 * L0 + w1 * L1) with
    LossBalancing's weights (loss_utils.py:303-318), re-weighted every step from its running score table (:320-345,
    trainer.py:640-642).  The weights are host scalars of the argument block and the table needs the step's two loss scalars
    on the host: eager launches, one device->host read per step (the reference makes 2 * bs of them, :316)."""
    from mal_amd import loss_utils
    st = Step(dev, seed, mode)
    st.lp.opt.loss_blc = True
    blc = loss_utils.LossBalancing(2, 1 << 20, B)
    lv = st.leaves

    def one(i):
        for t in lv.values():
            t.grad = None
        mono_outputs = {("disp", 0): lv["disp_teacher"]}
        for f, s_ in ((-1, "m1"), (1, "p1")):
            mono_outputs[("axisangle", 0, f)] = lv["axisangle_" + s_]
            mono_outputs[("translation", 0, f)] = lv["translation_" + s_]
        outputs = {("disp", 0): lv["disp_student"], "consistency_mask": st.cmask, "augmentation_mask": st.aug,
                   "lowest_cost": st.lowest}
        losses, loss_list, _ = st.step_mod.loss_step(st.lp.opt, st.inputs, mono_outputs, outputs, w_list=list(blc.w_list),
                                                     want_maps=False, image_synthesis=st.synth)
        losses["loss"].backward(gradient=st.one)
        blc.compute_loss(loss_list, i)      # the device->host read of the two scalars
        return blc.update_weight(i, 0.1)    # options.py: lambda_for_adjust_* ~ 0.1..0.3

    for i in range(5):
        one(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(5, 5 + steps):
        w = one(i)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    return {"ms_per_step": ms, "value": B / (ms * 1e-3), "unit": "images/s", "steps": steps, "launch": "eager",
            "w_ori": float(w[0]), "w_distil": float(w[1]),
            "what": "the step with --loss_blc: w_main = bs*w0, w_distil = bs*w1 in the argument block, LossBalancing.compute_loss "
                    "(one device->host read of the two loss scalars) and update_weight on the host after every step; compare "
                    "with eager_ms_per_step (the same eager step without it)"}


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        spawn_ranks(args)  # does not return
    global W
    W = args.width
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: the MAL loss path has no CPU fallback")
    # MAL_BENCH_BACKEND=gloo rehearses the N>1 launch on a box with fewer GPUs than ranks (ranks share devices)
    backend = os.environ.get("MAL_BENCH_BACKEND", "nccl")
    local = local % torch.cuda.device_count() if backend != "nccl" else local
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    from mal_amd import build, _lib
    if rank == 0:
        build.build(verbose=False)
    if dist is not None:
        dist.barrier()
    lib = _lib.load()
    for kv in args.opt:
        name, val = kv.split("=")
        _lib.check(lib.mal_set_option(name.encode(), int(val)), "mal_set_option(%s)" % kv)
    # regimes: cold = the timed passes rotate over R distinct batches (Rotation); warm = one batch replayed
    R = 1 if (args.regime == "warm" or args.mode == "train") else max(1, args.rotate)
    cold = R > 1
    both = cold and args.regime == "both"
    if args.mode == "train":
        step = TrainStep(dev, 1234 + rank)
        args.graph = 0  # host-side RNG, optimizer and collective in the step
        args.no_cpu_baseline = True
        rot = None
    else:
        rot = Rotation(dev, 1234 + rank, args.mode, R, graph=bool(args.graph), channels_last=args.channels_last,
                       main_temporal=args.main_temporal, ms_temporal=args.ms_temporal,
                       dr_scales=[0, 1, 2, 3] if args.dr_default_scales else None, dr_pose_update=args.dr_pose_update)
        step = rot.steps[0]
    batch_cpu = step.batch_cpu
    step_B = getattr(step, "B", B)  # images per rank and step (read here: the train_step block below frees `step`)

    def sync():
        # poll an event first: a blocking synchronize wakes the host up to ~0.1 ms late, which a short timed region
        # (small --steps) would be charged for; the barrier + synchronize the contract asks for follow
        e = torch.cuda.Event()
        e.record()
        while not e.query():
            pass
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    one_pass = rot if rot is not None else step
    eager_pass = rot.eager if rot is not None else step
    graph = rot.graphs if rot is not None else None
    graph_note = rot.note if rot is not None else None

    # N>1: the data-parallel exchange of the training step -- one all-reduce (mean) of the flat fp32 gradient bucket of
    # RepDepth (165 MB; mal_amd/dp.py, manydepth/trainer.py:309-311,469).  The loss path has no parameters of its own,
    # so outside --mode train (where the harness owns the real bucket) a buffer of the same size stands in for it.
    bucket = None
    if dist is not None and args.mode != "train":
        from mal_amd.dp import FlatGradBucket
        holder = torch.nn.Parameter(torch.zeros(N_GRAD_PARAMS, dtype=torch.float32,
                                                device=dev if backend == "nccl" else "cpu"))
        bucket = FlatGradBucket([holder])
        bucket.flat.normal_()

    def run():
        one_pass()
        if bucket is not None:
            bucket.all_reduce_mean()

    # bring the GPU to its sustained clocks first (a few warm-up steps of 0.2 ms do not): ~0.1 s of the same step,
    # untimed and independent of --warmup, so that a short --steps run measures the steady state too
    t_ramp = time.perf_counter()
    while args.mode != "train" and time.perf_counter() - t_ramp < 0.1:
        for _ in range(20):
            one_pass()
        torch.cuda.synchronize()
    # the ramp's length follows the clock: end it on a whole rotation and restart the tie-break noise streams, so that the
    # same arguments hand the timed steps the same batches and the same noise in every run (--dump-outputs compares runs)
    if rot is not None:
        while rot.i % R:
            rot()
        torch.cuda.synchronize()
        from mal_amd import step as step_mod
        step_mod.noise_counter(dev).zero_()
        torch.cuda.manual_seed(1234 + rank)
    for _ in range(args.warmup):
        run()
    # HIP events around the teacher-pass kernel (the first marching launch of a step), eager --full runs only
    ev = []
    sync()
    t0 = time.perf_counter()
    for i in range(args.steps):
        if args.full and graph is None and args.mode in ("step", "distil"):
            a, b_ = lib.mal_event_create(), lib.mal_event_create()
            lib.mal_profile_next_pass(a, b_)
            ev.append((a, b_))
        run()
    sync()
    dt = time.perf_counter() - t0
    n_ranks = world
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        n_ranks = dist.get_world_size()  # the ranks the collective actually saw
    # what the last timed step returned, read before any side measurement runs the step objects again
    outputs = None
    if args.dump_outputs and rank == 0:
        outputs = host_outputs(rot.steps[(rot.i - 1) % R] if rot is not None else step)

    # the WARM regime beside the line (rounds 1-4 reported this one): batch 0 replayed over and over, its ~100 MB working set
    # resident in the 256 MiB Infinity Cache
    warm_ms = None
    if args.full and both and rot is not None:
        n_w = max(args.steps, 100)
        for _ in range(20):
            rot.first()
        sync()
        t1 = time.perf_counter()
        for _ in range(n_w):
            rot.first()
        sync()
        warm_ms = 1e3 * (time.perf_counter() - t1) / n_w

    # the same step as eager launches (what a trainer whose producer cannot be captured into a graph would see: the
    # real producer calls two external models with a data-dependent number of instances between the library calls)
    eager_ms = None
    if args.full and graph is not None:
        n_e = max(args.steps, 50)
        for _ in range(5):
            eager_pass()
        sync()
        t1 = time.perf_counter()
        for _ in range(n_e):
            eager_pass()
            if bucket is not None:
                bucket.all_reduce_mean()
        sync()
        eager_ms = 1e3 * (time.perf_counter() - t1) / n_e

    # stages of the step, device time (HIP events on the current stream), outside the timed region
    breakdown = None
    if args.full and args.mode != "train":
        n_bd = 20
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        acc = [0.0, 0.0]
        for _ in range(n_bd):
            e[0].record()
            one_pass()
            e[1].record()
            if bucket is not None:
                bucket.all_reduce_mean()
            e[2].record()
            torch.cuda.synchronize()
            acc[0] += e[0].elapsed_time(e[1]) / n_bd
            acc[1] += e[1].elapsed_time(e[2]) / n_bd
        breakdown = {"loss_path_fwd_bwd": acc[0], "grad_all_reduce": acc[1] if bucket is not None else 0.0}

    # N>1, beside the headline (where every step WAITS for its exchange): the same steps with the exchange of step k in
    # flight on RCCL's stream while step k+1 computes -- how DDP hides it behind the backward (manydepth/trainer.py:469);
    # the loss path alone offers nothing else to hide 165 MB behind.  Reported as its own block, never as `value`.
    overlapped = None
    if args.full and bucket is not None:
        try:
            work = None
            sync()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                one_pass()
                if work is not None:
                    work.wait()
                work = bucket.all_reduce_mean(async_op=True)
            if work is not None:
                work.wait()
            sync()
            dt2 = time.perf_counter() - t1
            t = torch.tensor([dt2], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt2 = float(t.item())
            overlapped = {"value": world * B * args.steps / dt2, "unit": "images/s", "ms_per_step": 1e3 * dt2 / args.steps,
                          "what": "the same steps with each step's gradient all-reduce asynchronous on RCCL's stream, waited for "
                                  "one step later (at most one exchange in flight)"}
        except Exception as ex:  # the headline line must survive a failure of the side block
            overlapped = {"error": "%s: %s" % (type(ex).__name__, str(ex).splitlines()[0][:200])}

    durs = []
    if args.full and args.mode in ("step", "distil"):
        if graph is not None:  # kernel timing needs eager launches: a few extra steps outside the timed region
            for i in range(20):
                a, b_ = lib.mal_event_create(), lib.mal_event_create()
                lib.mal_profile_next_pass(a, b_)
                ev.append((a, b_))
                eager_pass()
            torch.cuda.synchronize()
        for a, b_ in ev:
            ms = ctypes.c_float(0)
            if lib.mal_event_elapsed_ms(a, b_, ctypes.byref(ms)) == 0:
                durs.append(ms.value)
            lib.mal_event_destroy(a), lib.mal_event_destroy(b_)
    kern_ms = sum(durs) / max(len(durs), 1)
    # the north-star kernel proper -- the fused warp+SSIM+L1+min+automask forward+backward sweep WITHOUT the temporal
    # hint's extra inputs (BASELINE's 96 B/px definition) -- timed in the same run: --distil steps of R_k batches of their own
    # (cold regime: 8 of them; warm: 1), first by events around eager launches, then replayed from a graph of nothing else
    kern_ms_plain = kern_ms
    replayed = replayed_warm = None
    if args.full and args.mode in ("step", "distil"):
        R_k = (8 if R >= 6 else R) if cold else 1  # (a reduced --rotate, as the quick tests use, reduces this rotation too)
        plains = Rotation(dev, 1234 + rank + 104729, "distil", R_k, slot_base=300, graph=False)
        pev = []
        for i in range(60):  # back to back (no host sync in between: the clocks stay where the timed region had them)
            a, b_ = lib.mal_event_create(), lib.mal_event_create()
            lib.mal_profile_next_pass(a, b_)
            plains.eager()
            pev.append((a, b_))
        torch.cuda.synchronize()
        pd = []
        for i, (a, b_) in enumerate(pev):
            ms = ctypes.c_float(0)
            if i >= 40 and lib.mal_event_elapsed_ms(a, b_, ctypes.byref(ms)) == 0:
                pd.append(ms.value)
            lib.mal_event_destroy(a), lib.mal_event_destroy(b_)
        kern_ms_plain = sum(pd) / max(len(pd), 1)
        # ... and the same kernel as a replayed graph runs it: a graph of nothing but 64 back-to-back launches, events outside
        try:
            enq = teacher_enqueuers(plains.steps, slot_base=100)
            replayed = replayed_kernel_ms(enq)
            if both:
                replayed_warm = replayed_kernel_ms(enq[:1])
            del enq
        except Exception as ex:  # the line survives (the eager-event figure then stands alone) and says why
            replayed = ("%s: %s" % (type(ex).__name__, str(ex).splitlines()[0][:200]),)
            torch.cuda.synchronize()
        del plains

    cl_block = None
    if args.full and args.mode in ("step", "distil") and not args.channels_last and rank == 0:
        try:
            cl_block = channels_last_block(dev, 1234 + rank, args.mode, R)
        except Exception as ex:
            cl_block = {"error": "%s: %s" % (type(ex).__name__, str(ex).splitlines()[0][:200])}
            torch.cuda.synchronize()
    # --loss-blc: the reference's own KITTI command (README.md:22) adds LossBalancing to the step
    blc_block = None
    if args.loss_blc and args.mode in ("step", "distil"):
        try:
            blc_block = loss_blc_block(dev, 1234 + rank, args.mode, max(args.steps, 50))
        except Exception as ex:
            blc_block = {"error": "%s: %s" % (type(ex).__name__, str(ex).splitlines()[0][:200])}
            torch.cuda.synchronize()

    # the whole training step (all ranks take part: its all-reduce is a collective).  With `value_is_train` (the default at
    # N>1) it IS the line: timed over exactly --steps steps after --warmup warm-ups, barrier + synchronize on both sides,
    # max over ranks; the loss-path measurement above then moves to the `loss_path` side block.
    # (round 5: `auto` no longer switches the quantity with N -- `value` is the loss path at every N, the whole training step
    # sits in `train_step` at every N, and `scaling_quantity` names the field the DP-scaling ratio is to be taken from)
    value_is_train = args.mode == "step" and args.value == "train"
    train_block = None
    if args.mode != "train" and ((args.full and args.train_steps > 0) or value_is_train):
        def train_side_block():
            nonlocal outputs
            n_train, n_warm = (args.steps, max(args.warmup, 1)) if value_is_train else (args.train_steps, 3)
            ts = TrainStep(dev, 1234 + rank)
            for _ in range(n_warm):
                ts()
            sync()
            t1 = time.perf_counter()
            for _ in range(n_train):
                ts()
            sync()
            dtt = time.perf_counter() - t1
            if value_is_train and args.dump_outputs and rank == 0:  # the line's timed path is this one
                outputs = host_outputs(ts)
            if dist is not None:
                t = torch.tensor([dtt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dtt = float(t.item())
            return {"value": n_ranks * B * n_train / dtt, "unit": "images/s", "ms_per_step": 1e3 * dtt / n_train,
                    "steps": n_train, "warmup": n_warm, "n_gpus": n_ranks, "breakdown_ms": ts.breakdown_ms(3),
                    "exchange": ts.h.exchange_note(), "exchange_pieces": len(ts.h.bucket.bounds),
                    "pieces_issued_inside_backward": int(ts.h.issued_inside_backward), "world_size": ts.h.bucket.world_size,
                    "what": "RepDepth (ResNet-18 x3 + decoders + pose + cost volume; fp32 torch.nn/MIOpen, random init) forward+backward, "
                            "this loss path (--temporal --distil, the producer's external models stubbed), the flat-bucket gradient "
                            "all-reduce launched from inside the backward, Adam; B=12 per GPU"}

        del step, graph, one_pass, eager_pass, rot
        torch.cuda.empty_cache()
        if dist is not None:
            train_block = train_side_block()  # N>1: a failing collective must fail the run
        else:
            try:
                train_block = train_side_block()
            except Exception as ex:  # N=1: the headline line survives a failure of the side block, and says so
                train_block = {"error": "%s: %s" % (type(ex).__name__, str(ex).splitlines()[0][:200])}

    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return
    n_px = B * H * W
    out = {
        "metric": "train images/sec at B=12 192x640 KITTI-shaped (MAL loss path: passes A+B+C fwd+bwd)",
        "value": n_ranks * step_B * args.steps / dt, "unit": "images/s", "n_gpus": n_ranks, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": ("ManyDepth+MAL loss step, B=12 per GPU, 192x640, --temporal --distil (teacher pass with the two "
                                "synthesised candidates of the temporal hint, ensemble + student passes, consistency + distillation "
                                "+ smoothness), fwd+bwd to disp/pose leaves incl. the gradient through syn; the hint's producer "
                                "(dyn_utils.image_synthesis, N2 kernels) runs inside the step with stand-ins for its two external "
                                "models, 3 matched instances per sample; scale 0 as the shipped decoder emits (SURVEY 9.1); "
                                "networks not included (see train_step)") if args.mode in ("step", "temporal") else
                               ("ManyDepth+MAL loss step, B=12 per GPU, 192x640, --distil (teacher+ensemble+student "
                                "passes, consistency+distillation+smoothness), fwd+bwd to disp/pose leaves; "
                                "networks not included (see train_step)"), "global_batch": B * n_ranks, "height": H, "width": W,
                   "parallelism": ("dp%d: replicas over disjoint batches, no data-path collective; every step ends with ONE RCCL "
                                   "all-reduce (mean) of the 165 MB flat fp32 gradient bucket" % n_ranks) if n_ranks > 1
                                  else "dp1 (single GPU: no collective)",
                   "launch": "hip-graph" if args.graph and graph_note is None else (graph_note or "eager"),
                   "clock_ramp": "0.1 s of untimed steps before the --warmup steps (sustained clocks)",
                   "api": {"step": "mal_loss_step_warp/_fwd/_bwd (three host calls around the producer)",
                           "distil": "mal_loss_step_fwd/_bwd (one host call per direction)",
                           "multiscale": "mal_loss_multiscale_fwd/_bwd (one host call per direction)"}.get(
                               args.mode, "operator-level (mal_amd.loss_utils / MALLossPath)")},
    }
    regime = "cold" if cold else "warm"
    out["config"]["regime"] = (
        "cold: the timed steps rotate over %d distinct synthetic batches, each with its own inputs, leaves and step workspace "
        "(~190 MB per batch: the 256 MiB Infinity Cache holds nothing of a batch when its turn comes again), so every operand "
        "of a step is fetched from HBM, as in a training step that runs 45 ms of convolutions between two loss calls "
        "(manydepth/trainer.py:465-470)" % R) if cold else (
        "warm: one synthetic batch replayed -- its ~100 MB working set stays in the 256 MiB Infinity Cache (what rounds 1-4 reported)")
    out["batches_rotated"] = R
    if args.mode != "train":
        out["%s_ms_per_step" % regime] = out["ms_per_step"]
        out["%s_value" % regime] = out["value"]
    if warm_ms is not None:
        out["warm_ms_per_step"] = warm_ms
        out["warm_value"] = n_ranks * step_B / (warm_ms * 1e-3)
    out["config"]["parity_gate"] = (
        "tests/test_gpu_decisions.py: decision-exact against the CPU oracle; loss scalars 1e-5 rel; every gradient at max(1e-4, 1.25 x "
        "the fp32 oracle's own distance from the fp64 oracle) -- plain 1e-4 at the golden sizes, at B=12 192x640 the reference's own "
        "fp32 arithmetic is 2e-4..6e-4 from exact on the pose gradients")
    if eager_ms is not None:
        out["eager_ms_per_step"] = eager_ms
        out["eager_value"] = n_ranks * step_B / (eager_ms * 1e-3)
    if blc_block is not None:
        out["loss_blc"] = blc_block
    if cl_block is not None:
        out["channels_last"] = cl_block
    if args.main_temporal and args.mode == "step":
        out["config"]["variant"] = "--main_temporal as well: the producer also runs on the student's warped images (MAL_STEP_MAIN_TEMPORAL)"
    if args.ms_temporal and args.mode == "multiscale":
        out["config"]["variant"] = "--temporal on the non-distil four-scale path: the producer once per scale (mal_loss_multiscale_warp)"
    out["config"]["input_layout"] = "channels_last (zero-copy texels)" if args.channels_last else "NCHW (the reference's tensors)"
    if breakdown is not None:
        out["breakdown_ms"] = breakdown
    if overlapped is not None:
        out["exchange_overlapped"] = overlapped
    if args.full and args.mode in ("step", "distil"):
        # kernel_ms / achieved / frac: the kernel inside a REPLAYED graph (what the headline's graph-replayed step runs),
        # measured in this run; eager_kernel_ms: the same kernel bracketed by HIP events on eager launches (6-10 % longer:
        # an eager stream's packets carry release fences, and the event pair adds packet processing; LABBOOK.md 5)
        have_replay = replayed is not None and len(replayed) == 2
        kernel_ms = replayed[0] if have_replay else kern_ms_plain
        frac_of = lambda ms: (ALG_BYTES_PER_PX * n_px / (ms * 1e-3) / 1e9) / HBM_PEAK_GBS if ms and ms > 0 else 0.0
        achieved = frac_of(kernel_ms) * HBM_PEAK_GBS
        copy_gbs = measured_copy_ceiling(dev)
        traffic = traffic_temporal = None
        tpath = os.path.join(ROOT, "profiles", "traffic.json")
        if os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                traffic, traffic_temporal = tj.get("pass_kernel_teacher_bytes_per_launch"), tj.get("pass_kernel_teacher_temporal_bytes_per_launch")
            except Exception:
                traffic = traffic_temporal = None
        n_b = (8 if R >= 6 else R) if cold else 1
        how_replay = ("a HIP graph holding ONLY 64 back-to-back launches of this kernel, launch i with the argument block of a "
                      "--distil step of batch i %% %d (mal_loss_step_teacher_replay; %s), replayed 10x after 2 warm-up replays, two "
                      "events outside the graph, / 640; includes the gaps between consecutive graph nodes"
                      % (n_b, ("%d batches x ~77 MB of operands: %d MB pass through the 256 MiB Infinity Cache between two launches "
                               "on the same batch%s" % (n_b, 77 * (n_b - 1), ", so every operand comes from HBM" if n_b >= 5 else
                                                        " -- NOT enough to evict it: a reduced --rotate")) if cold else
                              "one batch: its operands stay in the Infinity Cache"))
        out["roofline"] = {"bound": "hbm", "kernel": "mal::march_teacher_kernel<false> (teacher pass: warp+SSIM+L1+"
                                                     "min+automask fwd+bwd, one launch = the whole B=12 pass)",
                           "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                           "regime": regime,
                           "traffic": traffic,
                           "traffic_source": "profiles/traffic.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this kernel "
                                             "(2*FETCH+WRITE, gfx950 correction), committed with the round; not re-measured in this run",
                           "alg_bytes_per_px": ALG_BYTES_PER_PX, "pixels_per_launch": n_px,
                           "kernel_ms": kernel_ms,
                           "kernel_ms_how": how_replay if have_replay else
                                            ("HIP events around eager launches (the replayed measurement failed: %s)"
                                             % (replayed[0] if replayed else "not run")),
                           "launches_timed": replayed[1] if have_replay else 20,
                           "batches_rotated": n_b,
                           "eager_kernel_ms": kern_ms_plain, "eager_frac": frac_of(kern_ms_plain),
                           "eager_launches_timed": 20,
                           "measured_copy_GBs": copy_gbs, "frac_of_measured_copy": achieved / copy_gbs if copy_gbs else None}
        out["roofline"]["%s_kernel_ms" % regime] = kernel_ms
        out["roofline"]["%s_frac" % regime] = frac_of(kernel_ms)
        if replayed_warm is not None:
            out["roofline"]["warm_kernel_ms"] = replayed_warm[0]
            out["roofline"]["warm_frac"] = frac_of(replayed_warm[0])
        out["roofline"].update(valu_bound(lib, dev, kernel_ms, achieved / HBM_PEAK_GBS,
                                          halo1="march_halo1=0" not in args.opt))
    if args.mode == "step" and kern_ms > 0:
        # the same sweep as the headline step runs it: decisions of the four-way min taken from the materialised-candidate
        # kernels, + 24 B/px of d loss / d warped colour arriving through syn (SURVEY.md 8d counts +24 B/px backward)
        alg_t = ALG_BYTES_PER_PX + 24
        ach_t = alg_t * n_px / (kern_ms * 1e-3) / 1e9
        out["roofline_temporal"] = {"bound": "hbm", "kernel": "mal::march_teacher_kernel<true> (the teacher's gradient "
                                    "sweep inside the --temporal step)", "achieved": ach_t, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                    "frac": ach_t / HBM_PEAK_GBS, "traffic": traffic_temporal, "alg_bytes_per_px": alg_t,
                                    "pixels_per_launch": n_px, "kernel_ms": kern_ms, "launches_timed": len(durs)}
    if args.mode == "train":
        out["metric"] = "train images/sec at B=12 192x640 KITTI-shaped (whole training step of the harness)"
        out["config"]["workload"] = ("RepDepth (ResNet-18 x3 + decoders + pose, cost volume) forward+backward through torch.nn/MIOpen, "
                                     "MAL loss step (6 HIP kernels), one flat-bucket gradient all-reduce (165 MB fp32), Adam; "
                                     "B=12 per GPU, 192x640, --distil, synthetic batch, random-init weights")
        out["config"]["parallelism"] = "dp%d (one RCCL all-reduce of the flat gradient bucket per step)" % n_ranks
        out["config"]["api"] = "mal_amd.harness.TrainHarness.train_step"
        if args.full:
            out["breakdown_ms"] = step.breakdown_ms()
        out["exchange"] = step.h.exchange_note()
    elif args.mode in ("dualrefine", "dualrefine_ops"):
        out["config"]["workload"] = ("DualRefine+MAL loss loops, B=8 per GPU, 192x640 (BASELINE configs[4]): generate_images_pred + "
                                     "compute_losses over (scale 0, deq_iter 0..1), convention B warps (align_corners=False), fwd+bwd "
                                     "to disp/pose leaves; networks not included")
        out["config"]["api"] = ("mal_dr_loss_fwd/_bwd (one host call per direction)" if args.mode == "dualrefine"
                                else "operator-level (DualRefineLossPath.generate_images_pred + compute_losses)")
        out["config"]["global_batch"] = step_B * n_ranks
        out["metric"] = "train images/sec at B=8 192x640 KITTI-shaped (DualRefine+MAL loss loops, fwd+bwd)"
        if args.dr_pose_update:
            out["config"]["pose_updates"] = ("on: compute_pose_update_losses (dualrefine/trainer.py:457-480,699-767) as one more marching pass "
                                             "of the same call (MAL_DR_POSE_UPDATE)" if args.mode == "dualrefine" else
                                             "on: pose_update_generate_images_pred + compute_pose_update_losses through the operators")
        if args.dr_default_scales:
            out["config"]["variant"] = ("upstream's default scale list [0,1,2,3]: scale 0 and 2 with deq iterations 0..1, scale 1 skipped, "
                                        "scale 3 iteration 0 (one mal_dr_loss call per visited scale on the one-call route)")
    elif args.mode not in ("step", "distil"):
        out["config"]["workload"] += " [mode %s]" % args.mode
    if train_block is not None:
        out["train_step"] = train_block
        # the field the data-parallel scaling ratio is to be taken from, the same at every N (BASELINE's ">= 6x at 8 GPUs" is
        # about the whole training step; the loss path in `value` carries the trainer's 165 MB stand-in exchange after every
        # 0.3 ms step at N>1 and cannot exceed ~3x by construction)
        out["scaling_quantity"] = "train_step.value"
        out["world_size"] = n_ranks
    if value_is_train:
        # N>1 (or --value train): the line IS the whole training step -- the quantity BASELINE's ">= 6x DP scaling at 8 GPUs"
        # is about (the loss path alone cannot amortise the trainer's 165 MB exchange: DESIGN.md 5).  What the loss path
        # does beside the stand-in exchange moves to `loss_path`; roofline / cpu_baseline stay what they are.
        if "error" in train_block:
            raise SystemExit("bench.py: the training step failed: %s" % train_block["error"])
        side = {k: out.pop(k) for k in ("eager_ms_per_step", "eager_value", "breakdown_ms", "exchange_overlapped") if k in out}
        side.update(value=out["value"], unit="images/s", ms_per_step=out["ms_per_step"], steps=out["steps"], warmup=out["warmup"],
                    workload=out["config"]["workload"], launch=out["config"]["launch"], api=out["config"]["api"],
                    what="the loss path alone (graph-replayed) with the stand-in exchange of the trainer's 165 MB bucket after "
                         "every step: by construction <= ~3x at 8 GPUs (DESIGN.md 5), reported beside the line, never as it")
        out["loss_path"] = side
        out["metric"] = ("train images/sec at B=12 192x640 KITTI-shaped (whole training step: RepDepth fwd+bwd + MAL loss path "
                         "+ gradient all-reduce + Adam)")
        out["value"], out["ms_per_step"] = train_block["value"], train_block["ms_per_step"]
        out["steps"], out["warmup"] = train_block["steps"], train_block["warmup"]
        out["config"]["workload"] = ("RepDepth (ResNet-18 x3 + decoders + pose + cost volume; fp32 torch.nn/MIOpen, random init) "
                                     "forward+backward + this MAL loss path (--temporal --distil, the hint's producer with stand-ins "
                                     "for its two external models, 3 matched instances per sample) + ONE flat-bucket gradient "
                                     "all-reduce (mean, 165 MB fp32, issued in four pieces from inside the backward) + Adam; B=12 per GPU, "
                                     "192x640, synthetic batch")
        out["config"]["launch"] = "eager (host-side RNG, optimizer and collective in the step)"
        out["config"]["api"] = "mal_amd.harness.TrainHarness.train_step"
        out["value_is"] = "train_step (--value train): the line's value / ms_per_step are the whole training step's"
    if args.full and n_ranks == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(batch_cpu, args.cpu_steps, temporal=args.mode in ("step", "temporal"), seed=1234 + rank)
    if W != 640:  # --width: the strings above are written for the headline size
        def resize(o):
            if isinstance(o, str):
                return o.replace("192x640", "192x%d" % W).replace("KITTI-shaped", "CityScapes-shaped" if W == 512 else "KITTI-shaped")
            if isinstance(o, dict):
                return {k: resize(v) for k, v in o.items()}
            return o
        out = resize(out)
        out["config"]["width"] = W
    if outputs is not None:
        write_outputs(args.dump_outputs, outputs)
    print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
