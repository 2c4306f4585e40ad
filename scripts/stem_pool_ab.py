"""Same-box A/B of the stem max-pool kernels (mal_amd.glue.stem_pool) against the ATen route they replace.

    python scripts/stem_pool_ab.py [sites] [step] > profiles/stem_pool_ab.txt

sites: the stem pool of the three ResNet-18 encoders at B=12, 192x640 -- (12, 64, 96, 320) -> (12, 64, 48, 160) -- forward and
       backward, with and without the skip's cotangent, and the lookup frames' forward (no graph), the kernels against ATen, both
       through autograd as the model runs them: forward = the call with a graph, backward = torch.autograd.grad of (the stem
       feature as the decoder's skip reads it, the pooled map) w.r.t. the stem feature.  Either side costs the host more than
       the kernels take, so a call is timed inside a burst (scripts/encoder_glue_ab.py): a 7 ms matrix product is enqueued
       first, then an event, one call per buffer set, an event; every launch is queued while the product still runs and the
       events bracket device work alone.  The buffer sets are distinct and the product passes 768 MiB through the caches
       before each burst.  Medians of 50 bursts.  Beside each time: the bytes the route moves (counted from the shapes: every
       tensor a pass reads or writes, once) and bytes / time.
step:  bench.TrainStep with fused_pool set on the three encoders against unset, off / on / off / on, EACH ARM IN A FRESH CHILD
       PROCESS under its own `timeout -k 10`, 3 x 10 steps after 6 warm-ups, the median; the chain ends at the first child that
       does not exit with status 0.  The off arms are the parent commit's code path; the spread is their difference.
Nothing here is part of the test suite."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

COLD_BYTES = 256 << 20
B, C, H, W = 12, 64, 96, 320
ARM_SECONDS = 240


def route_bytes():
    """bytes each route moves per call, from the shapes: {(side, direction, skip cotangent): bytes}"""
    n_in, n_out = B * C * H * W, B * C * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)
    y, p = 4 * n_in, 4 * n_out
    code, index = n_out, 8 * n_out
    out = {}
    out["fused", "fwd"] = y + p + code          # read y; write p and one byte per output
    out["aten", "fwd"] = y + p + index          # read y; write p and an int64 index per output
    out["fused", "fwd_nograd"] = y + p
    out["aten", "fwd_nograd"] = y + p + index   # max_pool2d without a graph writes its indices too, into a buffer it drops
    out["fused", "bwd", True] = p + code + y + y            # read g_p, codes, g_y; write dy
    out["fused", "bwd", False] = p + code + y
    out["aten", "bwd", False] = y + p + index + 2 * p       # zero fill; read g_p, indices; one atomic read-modify-write per output
    out["aten", "bwd", True] = out["aten", "bwd", False] + 3 * y  # autograd's accumulation: two reads, one write
    return out


def measure_sites(reps=50, warm=3):
    from mal_amd.glue import stem_pool, stem_pool_plan
    dev = torch.device("cuda:0")
    ev = lambda: torch.cuda.Event(enable_timing=True)
    plug_a = torch.randn(8192, 8192, device=dev)
    plug = lambda: torch.mm(plug_a, plug_a)  # ~7 ms of device work: the host enqueues the burst behind it, and it evicts the caches

    def burst(calls):
        plug()
        s, e = ev(), ev()
        s.record()
        outs = [c() for c in calls]
        e.record()
        return s, e, outs

    n = B * C * H * W
    n_sets = min(16, max(2, -(-COLD_BYTES // (4 * n)) + 1))
    gen = torch.Generator(device=dev).manual_seed(1)
    xs = [torch.relu(torch.randn(B, C, H, W, device=dev, generator=gen)).requires_grad_(True) for _ in range(n_sets)]
    gys = [torch.randn(B, C, H, W, device=dev, generator=gen) for _ in range(n_sets)]
    gps = [torch.randn(B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1, device=dev, generator=gen) for _ in range(n_sets)]

    def fused_fwd(i):
        return stem_pool(xs[i])

    def aten_fwd(i):
        return xs[i].view_as(xs[i]), F.max_pool2d(xs[i], kernel_size=3, stride=2, padding=1)

    def bwd(i, outs, skip):
        y_out, p = outs[i]
        if skip:
            return torch.autograd.grad([y_out, p], [xs[i]], [gys[i], gps[i]])
        return torch.autograd.grad([p], [xs[i]], [gps[i]])

    def nograd(fn):
        def run(i):
            with torch.no_grad():
                return fn(i)
        return run

    t = {}
    for it in range(warm + reps):
        marks = {}
        for side, fwd in (("fused", fused_fwd), ("aten", aten_fwd)):
            for skip in (True, False):
                s0, e0, outs = burst([(lambda i=i: fwd(i)) for i in range(n_sets)])
                s1, e1, grads = burst([(lambda i=i: bwd(i, outs, skip)) for i in range(n_sets)])
                marks[side, "bwd", skip] = (s1, e1)
                if skip:
                    marks[side, "fwd"] = (s0, e0)
                del outs, grads
            s2, e2, outs = burst([(lambda i=i: nograd(fwd)(i)) for i in range(n_sets)])
            marks[side, "fwd_nograd"] = (s2, e2)
            del outs
        torch.cuda.synchronize()
        if it >= warm:
            for key, (s_, e_) in marks.items():
                t.setdefault(key, []).append(s_.elapsed_time(e_) * 1e3 / n_sets)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    nbytes = route_bytes()
    OH, OW, bf, bb, vf, vb = stem_pool_plan(B, C, H, W)
    print("stem pool (%d,%d,%d,%d) -> (%d,%d,%d,%d); kernels: %d workgroups x %d outputs per thread forward, %d x %d elements "
          "backward" % (B, C, H, W, B, C, OH, OW, bf, vf, bb, vb))
    print("device us per call (bursts of %d calls on distinct buffers behind a 7 ms plug, medians of %d bursts); MB moved by the "
          "route's passes, counted from the shapes; TB/s = MB / us" % (n_sets, reps))
    print("%-42s | %8s %7s %6s | %8s %7s %6s | %5s" % ("site", "fused us", "MB", "TB/s", "ATen us", "MB", "TB/s", "x"))
    rows = (("forward, graph (codes / indices saved)", ("fwd",)), ("forward, no graph (lookup frames, val)", ("fwd_nograd",)),
            ("backward with the skip's cotangent", ("bwd", True)), ("backward, pool's cotangent alone", ("bwd", False)))
    for name, key in rows:
        f, a = med[("fused",) + key], med[("aten",) + key]
        fb, ab = nbytes[("fused",) + key], nbytes[("aten",) + key]
        print("%-42s | %8.1f %7.1f %6.2f | %8.1f %7.1f %6.2f | %5.2f" % (name, f, fb / 1e6, fb / f / 1e6, a, ab / 1e6, ab / a / 1e6, a / f),
              flush=True)
    per_enc_f = med["fused", "fwd"] + med["fused", "bwd", True]
    per_enc_a = med["aten", "fwd"] + med["aten", "bwd", True]
    print("one encoder whose stem feature is a decoder skip, forward + backward: fused %.0f us, ATen %.0f us" % (per_enc_f, per_enc_a))
    print("a step (two such encoders, the pose encoder without a skip, the lookup frames' forward): fused %.0f us, ATen %.0f us"
          % (2 * per_enc_f + med["fused", "fwd"] + med["fused", "bwd", False] + med["fused", "fwd_nograd"],
             2 * per_enc_a + med["aten", "fwd"] + med["aten", "bwd", False] + med["aten", "fwd_nograd"]), flush=True)


def step_arm(on):
    """one arm, in this (fresh) process: prints the median ms per step"""
    sys.argv = sys.argv[:1]
    import bench
    dev = torch.device("cuda:0")
    st = bench.TrainStep(dev, 1234)
    for enc in (st.h.model.encoder, st.h.model.mono_encoder, st.h.model.pose_encoder):
        enc.fused_pool = on
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
        p = subprocess.run(["timeout", "-k", "10", str(ARM_SECONDS), sys.executable, os.path.abspath(__file__), "arm-" + tag], cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("ARM ")]
        if p.returncode != 0 or not line:
            print("train_step fused_pool %-3s  no result: the child exited with status %d%s; the chain ends here\n%s"
                  % (tag, p.returncode, " (its %d s limit)" % ARM_SECONDS if p.returncode in (124, 137) else "",
                     "\n".join(p.stdout.splitlines()[-15:])))
            return 1
        f = line[-1].split()
        res.append((tag, float(f[2])))
        print("train_step fused_pool %-3s  %.2f ms per step  (%s)  [fresh process]" % (tag, float(f[2]), ", ".join(f[3:])), flush=True)
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
