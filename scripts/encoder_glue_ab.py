"""Same-box A/B of the fused encoder glue (mal_amd.glue.bn_join) against the ATen/MIOpen chain it replaces.

    python scripts/encoder_glue_ab.py [sites] [step] > profiles/encoder_glue_ab.txt

sites: every distinct BatchNorm2d -> (+ identity) -> ReLU site shape of the three ResNet-18 encoders at B=12, 192x640, forward
       and backward, fused against ATen, device events, medians of 50.  Both sides run through autograd as the model runs them
       (forward = the module call(s) with a graph, backward = torch.autograd.grad of the output w.r.t. x, the residual, gamma and
       beta), and either side costs the host 45-120 us per call -- more than most of these kernels take.  Events around ONE call
       therefore time the host, not the device (and time it unevenly: the side whose forward kernels are slower hides more of
       its backward's enqueue).  So a call is timed inside a burst: a 7 ms matrix product is enqueued first, then an event, one
       call per buffer set, an event; every launch is queued while the product still runs, and the events bracket device work
       alone.  The buffer sets are distinct and the product passes 768 MiB through the caches before each burst (the cold
       regime of DESIGN.md 5; up to 16 sets, more than 256 MiB where the site is large enough to matter).
step:  bench.TrainStep with fused_glue set on the three encoders against unset, off / on / off / on, EACH ARM IN A FRESH CHILD
       PROCESS under a time limit, 3 x 10 steps after 6 warm-ups, the median; the chain ends at the first child
       that does not exit with status 0.  The spread is the difference of the two "off" runs.
Nothing here is part of the test suite."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn as nn
import torch.nn.functional as F

COLD_BYTES = 256 << 20
B, IMG_H, IMG_W = 12, 192, 640
ARM_SECONDS = 240


def sites():
    """(name, C, H, W, residual, relu, uses per ResNet-18) in forward order"""
    out = [("stem.bn1", 64, IMG_H // 2, IMG_W // 2, 0, 1, 1)]
    for i, c in enumerate((64, 128, 256, 512)):
        h, w = IMG_H >> (i + 2), IMG_W >> (i + 2)
        out.append(("layer%d.bn1" % (i + 1), c, h, w, 0, 1, 2))
        out.append(("layer%d.bn2" % (i + 1), c, h, w, 1, 1, 2))
        if i:
            out.append(("layer%d.downsample" % (i + 1), c, h, w, 0, 0, 1))
    return out


def aten_chain(x, bn, r, relu):
    """what BasicBlock.forward / the stem run behind the convolution; the ReLU is in place as nn.ReLU(inplace=True) is"""
    out = bn(x)
    if r is not None:
        out = out + r
    return F.relu_(out) if relu else out


def measure_sites(reps=50, warm=3):
    from mal_amd.glue import bn_join, bn_join_plan
    dev = torch.device("cuda:0")
    ev = lambda: torch.cuda.Event(enable_timing=True)
    plug_a = torch.randn(8192, 8192, device=dev)
    plug = lambda: torch.mm(plug_a, plug_a)  # ~7 ms of device work: the host enqueues the burst behind it, and it evicts the caches

    def burst(calls):
        """device time of the calls alone: both events and every launch between them are queued while the plug still runs"""
        plug()
        s, e = ev(), ev()
        s.record()
        outs = [c() for c in calls]
        e.record()
        return s, e, outs

    print("device us per call (bursts of `sets` calls on distinct buffers behind a 7 ms plug, medians of %d bursts)" % reps)
    print("site               C    H    W res relu uses blocks sets |  fwd us: fused   ATen    x |  bwd us: fused   ATen    x | MB of x")
    total = {"ff": 0.0, "fa": 0.0, "bf": 0.0, "ba": 0.0}
    for name, C, H, W, res, relu, uses in sites():
        n = B * C * H * W
        n_sets = min(16, max(2, -(-COLD_BYTES // (4 * n)) + 1))
        gen = torch.Generator(device=dev).manual_seed(1)
        xs = [torch.randn(B, C, H, W, device=dev, generator=gen).requires_grad_(True) for _ in range(n_sets)]
        rs = [torch.randn(B, C, H, W, device=dev, generator=gen).requires_grad_(True) if res else None for _ in range(n_sets)]
        gs = [torch.randn(B, C, H, W, device=dev, generator=gen) for _ in range(n_sets)]
        bn_f, bn_a = nn.BatchNorm2d(C).to(dev), nn.BatchNorm2d(C).to(dev)
        wrt = lambda i, bn: [xs[i]] + ([rs[i]] if res else []) + [bn.weight, bn.bias]
        t = {k: [] for k in total}
        for it in range(warm + reps):
            marks = {}
            for tag, bn, fwd in (("f", bn_f, lambda i: bn_join(xs[i], bn_f, rs[i], bool(relu))),
                                 ("a", bn_a, lambda i: aten_chain(xs[i], bn_a, rs[i], relu))):
                s0, e0, ys = burst([(lambda i=i: fwd(i)) for i in range(n_sets)])
                s1, e1, grads = burst([(lambda i=i: torch.autograd.grad(ys[i], wrt(i, bn), gs[i])) for i in range(n_sets)])
                marks["f" + tag], marks["b" + tag] = (s0, e0), (s1, e1)
                del ys, grads
            torch.cuda.synchronize()
            if it >= warm:
                for key, (s_, e_) in marks.items():
                    t[key].append(s_.elapsed_time(e_) * 1e3 / n_sets)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        for k in total:
            total[k] += uses * med[k]
        print("%-16s %4d %4d %4d   %d    %d    %d   %4d %4d | %14.1f %6.1f %4.2f | %14.1f %6.1f %4.2f | %7.1f"
              % (name, C, H, W, res, relu, uses, bn_join_plan(B, C, H, W)[0], n_sets, med["ff"], med["fa"], med["fa"] / med["ff"],
                 med["bf"], med["ba"], med["ba"] / med["bf"], 4 * n / 1e6), flush=True)
        del xs, rs, gs
        torch.cuda.empty_cache()
    print("one ResNet-18 at B=%d (sum of uses x median): fwd fused %.0f us ATen %.0f us | bwd fused %.0f us ATen %.0f us"
          % (B, total["ff"], total["fa"], total["bf"], total["ba"]), flush=True)


def step_arm(on):
    """one arm, in this (fresh) process: prints the median ms per step"""
    sys.argv = sys.argv[:1]
    import bench
    dev = torch.device("cuda:0")
    st = bench.TrainStep(dev, 1234)
    for enc in (st.h.model.encoder, st.h.model.mono_encoder, st.h.model.pose_encoder):
        enc.fused_glue = on
    for _ in range(6):
        st()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(10):
            st()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / 10 * 1e3)
    print("ARM %s %.3f %s" % ("on" if on else "off", sorted(ts)[1], " ".join("%.3f" % v for v in ts)), flush=True)


def measure_step():
    res = []
    for tag in ("off", "on", "off", "on"):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "arm-" + tag], cwd=ROOT, stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, text=True, timeout=ARM_SECONDS)
        except subprocess.TimeoutExpired:
            print("train_step fused_glue %-3s  no result: the child passed its %d s limit; the chain ends here" % (tag, ARM_SECONDS))
            return 1
        line = [l for l in p.stdout.splitlines() if l.startswith("ARM ")]
        if p.returncode != 0 or not line:
            print("train_step fused_glue %-3s  no result: the child exited with status %d; the chain ends here\n%s"
                  % (tag, p.returncode, "\n".join(p.stdout.splitlines()[-15:])))
            return 1
        f = line[-1].split()
        res.append((tag, float(f[2])))
        print("train_step fused_glue %-3s  %.2f ms per step  (%s)  [fresh process]" % (tag, float(f[2]), ", ".join(f[3:])), flush=True)
    off = [v for k, v in res if k == "off"]
    on = [v for k, v in res if k == "on"]
    spread = abs(off[0] - off[1])
    gain = sum(off) / 2 - sum(on) / 2
    print("spread of the two off runs %.2f ms; mean off - mean on = %.2f ms -> %s"
          % (spread, gain, "on wins by more than the spread" if gain > spread else "no win beyond the spread"))
    return 0


if __name__ == "__main__":
    which = sys.argv[1:] or ["sites", "step"]
    if which[0] in ("arm-off", "arm-on"):
        step_arm(which[0] == "arm-on")
        sys.exit(0)
    print("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__, flush=True)
    rc = 0
    if "sites" in which:
        measure_sites()
    if "step" in which:
        rc = measure_step()
    sys.exit(rc)
