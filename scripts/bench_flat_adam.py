"""Same-box measurement of the flat Adam step (mal_amd.optim.FlatAdam, mal_amd/csrc/mal_adam.hip) against the torch routes.

    python scripts/bench_flat_adam.py [kernel] [step] > profiles/flat_adam.txt

kernel: the optimizer step alone on RepDepth's real parameter list (234 tensors, 41.2 M fp32) on one GPU, separate timed
        regions in one process for torch.optim.Adam as the harness builds it (foreach / multi_tensor_apply: the parent's
        behaviour), torch.optim.Adam(fused=True), FlatAdam.step(), FlatAdam.step(zero_grad=True) and the bare flat.zero_()
        the bucket pays per step.  The four streams (p, g, m, v) total 660 MB, more than the 256 MiB Infinity Cache, so a
        back-to-back loop is already the cold regime: a region is 20 steps between two device events, 9 regions per arm after
        5 warm-up steps, the arms interleaved region by region; median, minimum and maximum per step.  Bytes are counted from
        the shapes (28 per parameter: read p, g, m, v, write p, m, v; 32 with zero_grad; 4 for the memset) and the rate is
        given against 6.3 TB/s (achievable) and 8 TB/s (peak); for the torch routes the rate is what the same 28 bytes would
        mean at their time -- they move more.
step:   TrainHarness.train_step at B=12, 192x640, --temporal --distil (the configuration bench.py --mode train times) with
        fused_adam off / on / off / on, EACH ARM IN A FRESH CHILD PROCESS under its own `timeout -k 10`: 3 x 10 steps after 6
        warm-ups (median, host clock around a synchronise), then 5 steps with stage marks (mean device ms per stage; the
        bucket's memset falls into "networks_fwd", the optimizer into "adam").  The chain ends at the first child that does not
        exit with status 0.  The off arms are the parent's code path; the spread is their difference.
Nothing here is part of the test suite, and no pass/fail number is attached to the speed."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

B, H, W = 12, 192, 640
ARM_SECONDS = 300
REGION_STEPS, REGIONS, WARM = 20, 9, 5


def measure_kernel():
    from mal_amd import dp, harness, networks
    from mal_amd.optim import FlatAdam, adam_plan
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = networks.RepDepth(harness.default_options()).to(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    bucket = dp.FlatGradBucket(params)
    n = bucket.flat.numel()
    gen = torch.Generator(device=dev).manual_seed(1)
    grads = torch.randn(n, device=dev, generator=gen) * 1e-3

    arms = {}
    foreach = torch.optim.Adam(params, 1e-4)
    arms["torch.optim.Adam (foreach: the parent's)"] = (foreach.step, 28)
    try:
        fused = torch.optim.Adam(params, 1e-4, fused=True)
        arms["torch.optim.Adam(fused=True)"] = (fused.step, 28)
    except Exception as ex:  # a torch build without the fused implementation
        print("torch.optim.Adam(fused=True) is not available here: %s" % ex)
    flat = FlatAdam(params, bucket, 1e-4)
    arms["FlatAdam.step()"] = (flat.step, 28)
    arms["FlatAdam.step(zero_grad=True)"] = (lambda: flat.step(zero_grad=True), 32)
    arms["flat.zero_() (the bucket's memset)"] = (bucket.flat.zero_, 4)

    ev = lambda: torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in arms}
    for fn, _ in arms.values():
        bucket.flat.copy_(grads)
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    for _ in range(REGIONS):
        for name, (fn, _) in arms.items():
            bucket.flat.copy_(grads)  # every region starts from the same gradients (zero_grad and the memset clear them)
            s, e = ev(), ev()
            s.record()
            for _ in range(REGION_STEPS):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / REGION_STEPS)
    pl = adam_plan(len(params), n)
    print("optimizer step alone: %d tensors, %d fp32 parameters (%.0f MB per stream, %.0f MB over p, g, m, v: past the 256 MiB "
          "Infinity Cache, a back-to-back loop is the cold regime)" % (len(params), n, 4 * n / 1e6, 16 * n / 1e6))
    print("mal_adam_flat: one launch of %d workgroups x %d threads, tiles of %d elements" % (pl["blocks"], pl["threads"], pl["tile_elements"]))
    print("device us per step: regions of %d back-to-back steps between two events, %d regions per arm after %d warm-up steps, arms "
          "interleaved; MB counted from the shapes" % (REGION_STEPS, REGIONS, WARM))
    print("%-42s | %9s %9s %9s | %7s %6s | %9s %7s" % ("arm", "median us", "min us", "max us", "MB", "TB/s", "of 6.3", "of 8"))
    for name, (_, bpp) in arms.items():
        v = sorted(times[name])
        med = v[len(v) // 2]
        mb = bpp * n / 1e6
        rate = mb / med  # MB / us = TB/s
        note = "" if name.startswith(("FlatAdam", "flat")) else "  (rate: the 28 B/parameter of one pass at this time)"
        print("%-42s | %9.1f %9.1f %9.1f | %7.0f %6.2f | %8.0f%% %6.0f%%%s" % (name, med, v[0], v[-1], mb, rate, 100 * rate / 6.3,
                                                                            100 * rate / 8.0, note), flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    mine = med["FlatAdam.step()"]
    others = [v for k, v in med.items() if k.startswith("torch")]
    print("FlatAdam.step() is %s both torch routes (%.1f us against %s)" % (
        "faster than" if all(mine < o for o in others) else "NOT faster than", mine, ", ".join("%.1f" % o for o in others)))
    saved = med["torch.optim.Adam (foreach: the parent's)"] + med["flat.zero_() (the bucket's memset)"] - med["FlatAdam.step(zero_grad=True)"]
    print("per step, foreach Adam + memset - FlatAdam.step(zero_grad=True) = %.1f us" % saved, flush=True)


def step_arm(on):
    """one arm, in this (fresh) process"""
    import random
    from mal_amd import config, dyn_utils, harness
    from mal_amd.synthetic import instance_stub
    dev = torch.device("cuda:0")
    config.noise_source = "cuda"
    random.seed(1234)
    torch.manual_seed(1234)
    opt = harness.default_options(batch_size=B, height=H, width=W, temporal=True, fused_adam=on)
    ins_model, matcher = instance_stub(B, H, W, n_inst=3, seed=1234, device=dev)
    synth = lambda inputs, outputs, scale: dyn_utils.image_synthesis(inputs, outputs, scale, 0.5, ins_model, matcher)
    h = harness.TrainHarness(opt, dev, image_synthesis=synth)
    inputs = harness.synthetic_inputs(opt, dev, seed=1234)
    for _ in range(6):
        h.train_step(inputs)
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(10):
            h.train_step(inputs)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / 10 * 1e3)
    acc = {}
    for _ in range(5):
        t = harness.StageTimer()
        h.train_step(inputs, t)
        for k, v in t.result_ms().items():
            acc[k] = acc.get(k, 0.0) + v / 5
    print("ARM %s %.3f %s | %s" % ("on" if on else "off", sorted(ts)[1], " ".join("%.3f" % v for v in ts),
                                   " ".join("%s=%.3f" % kv for kv in acc.items())), flush=True)


def measure_step():
    res = []
    for tag in ("off", "on", "off", "on"):
        p = subprocess.run(["timeout", "-k", "10", str(ARM_SECONDS), sys.executable, os.path.abspath(__file__), "arm-" + tag], cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("ARM ")]
        if p.returncode != 0 or not line:
            print("train_step fused_adam %-3s  no result: the child exited with status %d%s; the chain ends here\n%s"
                  % (tag, p.returncode, " (its %d s limit)" % ARM_SECONDS if p.returncode in (124, 137) else "",
                     "\n".join(p.stdout.splitlines()[-15:])))
            return 1
        head, stages = line[-1].split(" | ")
        f = head.split()
        res.append((tag, float(f[2])))
        print("train_step fused_adam %-3s  %.2f ms per step  (%s)  stages, device ms: %s  [fresh process]"
              % (tag, float(f[2]), ", ".join(f[3:]), stages), flush=True)
    off = [v for k, v in res if k == "off"]
    on = [v for k, v in res if k == "on"]
    spread = max(abs(off[0] - off[1]), abs(on[0] - on[1]))
    gain = sum(off) / 2 - sum(on) / 2
    print("spread of two runs of the same arm %.2f ms; mean off - mean on = %.2f ms -> %s"
          % (spread, gain, "on wins by more than the spread" if gain > spread else "no win beyond the spread"))
    return 0


if __name__ == "__main__":
    which = sys.argv[1:] or ["kernel", "step"]
    if which[0] in ("arm-off", "arm-on"):
        step_arm(which[0] == "arm-on")
        sys.exit(0)
    print("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__, flush=True)
    rc = 0
    if "kernel" in which:
        measure_kernel()
    if "step" in which:
        rc = measure_step()
    sys.exit(rc)
