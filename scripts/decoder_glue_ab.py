"""Same-box A/B of the fused decoder glue (mal_amd.glue.decoder_join) against the ATen chain it replaces.

    python scripts/decoder_glue_ab.py [sites] [step] > profiles/decoder_glue_ab.txt

sites: the 11 padding sites of one DepthDecoder at B=12, 192x640, forward and backward, device events around each call,
       the fused call and the ATen chain alternating, >= 50 repetitions each after warm-up, the inputs rotating over enough
       buffer sets that more than 256 MiB passes between two uses of a buffer (the cold regime of DESIGN.md 5).  Bytes are
       the algorithmic ones: 4 * (B*C*h*w + B*Cs*H*W + B*(C+Cs)*(H+2)*(W+2)) each way.
step:  bench.TrainStep with fused_glue set on both decoders against unset, off / on / off / on, each 3 x 10 steps after 6
       warm-ups (scripts/train_variants.py); the spread is the difference of the two "off" runs.
One process; nothing here is part of the test suite."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

PEAK = 6.3e12  # plain-copy rate, bytes per second
COLD_BYTES = 256 << 20
B, IMG_H, IMG_W = 12, 192, 640
NUM_CH_ENC, NUM_CH_DEC = [64, 64, 128, 256, 512], [16, 32, 64, 128, 256]


def sites():
    """(name, C, Cs, h, w, up, elu) in forward order"""
    out = []
    size = lambda lvl: (IMG_H >> (lvl + 1), IMG_W >> (lvl + 1))  # encoder feature `lvl`
    for i in range(4, -1, -1):
        h, w = size(i)
        c_in = NUM_CH_ENC[-1] if i == 4 else NUM_CH_DEC[i + 1]
        out.append(("upconv_%d_0" % i, c_in, 0, h, w, 1, int(i != 4)))
        out.append(("upconv_%d_1" % i, NUM_CH_DEC[i], NUM_CH_ENC[i - 1] if i > 0 else 0, h, w, 2, 1))
    out.append(("dispconv_0", NUM_CH_DEC[0], 0, IMG_H, IMG_W, 1, 1))
    return out


def aten_forward(x, skip, up, elu):
    """what DepthDecoder.forward runs between two convolutions; the ELU is in place on the convolution's output"""
    y = F.elu(x, inplace=True) if elu else x
    if up == 2:
        y = F.interpolate(y, scale_factor=2, mode="nearest")
    if up == 2:  # torch.cat runs at these sites even with one element
        y = torch.cat([y, skip] if skip is not None else [y], 1)
    return F.pad(y, (1, 1, 1, 1), mode="reflect"), y


def aten_backward(g, cat_out, y_act, C, h, w, up, elu):
    """the nodes autograd runs for that chain: reflection-pad backward, the narrow views of cat's backward, nearest-upsampling
    backward, ELU backward from its result"""
    a = torch.ops.aten
    gc = a.reflection_pad2d_backward(g, cat_out, [1, 1, 1, 1])
    gx, gs = gc, None
    if up == 2:
        gx, gs = gc[:, :C], (gc[:, C:] if gc.shape[1] > C else None)
        gx = a.upsample_nearest2d_backward(gx, [up * h, up * w], [g.shape[0], C, h, w], 2.0, 2.0)
    if elu:
        gx = a.elu_backward(gx, 1.0, 1.0, 1.0, True, y_act)
    return gx, gs


def measure_sites(reps=50, warm=5, batch=B):
    from mal_amd.glue import decoder_join_bwd, decoder_join_fwd
    dev = torch.device("cuda:0")
    ev = lambda: torch.cuda.Event(enable_timing=True)
    print("site              C   Cs    h    w up elu sets |  fwd us: fused   ATen  x   share |  bwd us: fused   ATen  x   share | MB each way")
    for name, C, Cs, h, w, up, elu in sites():
        H, W = up * h, up * w
        n_x, n_s, n_o = batch * C * h * w, batch * Cs * H * W, batch * (C + Cs) * (H + 2) * (W + 2)
        nbytes = 4 * (n_x + n_s + n_o)
        n_sets = max(2, -(-COLD_BYTES // (4 * (n_x + n_s))) + 1, -(-COLD_BYTES // (4 * n_o)) + 1)
        gen = torch.Generator(device=dev).manual_seed(1)
        xs = [3 * torch.randn(batch, C, h, w, device=dev, generator=gen) for _ in range(n_sets)]
        ss = [torch.randn(batch, Cs, H, W, device=dev, generator=gen) if Cs else None for _ in range(n_sets)]
        gs = [torch.randn(batch, C + Cs, H + 2, W + 2, device=dev, generator=gen) for _ in range(n_sets)]
        t = {k: [] for k in ("ff", "fa", "bf", "ba")}
        with torch.no_grad():
            for it in range(warm + reps):
                k = it % n_sets
                k2 = (it + n_sets // 2) % n_sets
                e = [ev() for _ in range(8)]
                # fused
                e[0].record()
                out = decoder_join_fwd(xs[k], ss[k], up, bool(elu))
                e[1].record()
                del out
                e[2].record()
                gx, gk = decoder_join_bwd(gs[k], xs[k] if elu else None, Cs, up, bool(elu), True, True, (batch, C, h, w))
                e[3].record()
                del gx, gk
                # ATen, on a buffer set half a rotation away
                xin = xs[k2]
                e[4].record()
                padded, cat_out = aten_forward(xin, ss[k2], up, elu)
                e[5].record()
                del padded
                e[6].record()
                gx, gk = aten_backward(gs[k2], cat_out, xin, C, h, w, up, elu)
                e[7].record()
                del gx, gk, cat_out
                torch.cuda.synchronize()
                if it >= warm:
                    for key, a, b_ in (("ff", 0, 1), ("bf", 2, 3), ("fa", 4, 5), ("ba", 6, 7)):
                        t[key].append(e[a].elapsed_time(e[b_]) * 1e3)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        share = lambda us: 100.0 * nbytes / (us * 1e-6) / PEAK
        print("%-14s %4d %4d %4d %4d  %d   %d %4d | %14.1f %6.1f %4.2f %5.1f%% | %14.1f %6.1f %4.2f %5.1f%% | %7.1f"
              % (name, C, Cs, h, w, up, elu, n_sets, med["ff"], med["fa"], med["fa"] / med["ff"], share(med["ff"]),
                 med["bf"], med["ba"], med["ba"] / med["bf"], share(med["bf"]), nbytes / 1e6), flush=True)
        del xs, ss, gs
        torch.cuda.empty_cache()


def measure_step():
    import bench
    dev = torch.device("cuda:0")
    st = bench.TrainStep(dev, 1234)
    decoders = (st.h.model.depth, st.h.model.mono_depth)
    res = []
    for tag, on in (("off", False), ("on", True), ("off", False), ("on", True)):
        for d in decoders:
            d.fused_glue = on
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
        res.append((tag, sorted(ts)[1]))
        print("train_step fused_glue %-3s  %.2f ms per step  (%s)" % (tag, sorted(ts)[1], ", ".join("%.2f" % v for v in ts)), flush=True)
    off = [v for k, v in res if k == "off"]
    on = [v for k, v in res if k == "on"]
    spread = abs(off[0] - off[1])
    gain = sum(off) / 2 - sum(on) / 2
    print("spread of the two off runs %.2f ms; mean off - mean on = %.2f ms -> %s"
          % (spread, gain, "on wins by more than the spread" if gain > spread else "no win beyond the spread"))


if __name__ == "__main__":
    which = sys.argv[1:] or ["sites", "step"]
    print("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__, flush=True)
    if "sites" in which:
        measure_sites()
    if "step" in which:
        measure_step()
