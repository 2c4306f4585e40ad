"""Multi-scale deformable attention (mal_amd/msda.py) at the segmenter's shape for this project's images, on one MI355X:

    python scripts/msda_bench.py [launches per graph]      # prints; profiles/msda_bench.txt is a copy of the output

N = 12, levels 24x80, 12x40, 6x20 (S = Lq = 2520, the pixel decoder's self-attention), M = 8, D = 32, P = 4.  Four routes,
on the same box, inputs and process:

    plain        mal_msda_fwd on given locations and weights
    fused        mal_msda_fused_fwd on the linear layers' raw offsets and logits + reference points
    ATen + plain softmax and the location arithmetic as torch operators (three passes), then the plain kernel: what
                 fused=False costs, the figure `fused` has to beat
    grid_sample  the fallback formula (one F.grid_sample per level, stack, product, sum) as torch operators

Each is measured as DESIGN.md 5 measures the teacher pass: ONE captured graph of back-to-back launches, launch i on argument
block i mod B, replayed between two events outside the graph.  Cold: B = 8 distinct argument blocks (8 x ~97 MB, far beyond
the 256 MiB Infinity Cache); warm: B = 1.  Median and spread of ROUNDS such measurements, the routes alternating.
Byte floor: value + locations + weights + output, each read or written once, over the 8 TB/s peak."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from mal_amd import msda

DEV = torch.device("cuda:0")
PER_GRAPH = max(int(sys.argv[1]) if len(sys.argv) > 1 else 64, 8)
REPLAYS, ROUNDS, BLOCKS, PEAK = 10, 7, 8, 8.0e12
N, M, D, P = 12, 8, 32, 4
LEVELS = ((24, 80), (12, 40), (6, 20))
L = len(LEVELS)
S = sum(h * w for h, w in LEVELS)
LQ = S


def grid_sample_route(value, loc, weights):
    """the same sum through F.grid_sample (bilinear, zero padding, align_corners=False at 2 x - 1), level by level"""
    per_level, at = [], 0
    for l, (h, w) in enumerate(LEVELS):
        plane = value[:, at:at + h * w].permute(0, 2, 3, 1).reshape(N * M, D, h, w)
        at += h * w
        grid = (2.0 * loc[:, :, :, l] - 1.0).permute(0, 2, 1, 3, 4).reshape(N * M, LQ, P, 2)
        per_level.append(F.grid_sample(plane, grid, mode="bilinear", padding_mode="zeros", align_corners=False))
    sampled = torch.cat(per_level, -1)                                  # (N M, D, Lq, L P), level-major like the weights
    wt = weights.permute(0, 2, 1, 3, 4).reshape(N * M, 1, LQ, L * P)
    return (sampled * wt).sum(-1).view(N, M * D, LQ).permute(0, 2, 1).contiguous()


def aten_prep(offsets, logits, ref, wh):
    weights = torch.softmax(logits, -1).view(N, LQ, M, L, P)
    loc = ref[:, :, None, :, None, :] + offsets / wh[None, None, None, :, None, :]
    return loc, weights


def make_block(seed, shapes, start, wh):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    value = r(N, S, M, D)
    ref = torch.rand(N, LQ, 1, 2, device=DEV, generator=g).expand(N, LQ, L, 2).contiguous()
    offsets = r(N, LQ, M, L, P, 2) * 2.0  # pixels: a few texels around the query, as the decoder's offsets
    logits = r(N, LQ, M, L * P)
    loc, weights = aten_prep(offsets, logits, ref, wh)
    return dict(value=value, ref=ref, offsets=offsets, logits=logits, loc=loc.contiguous(), weights=weights.contiguous(),
                shapes=shapes, start=start, wh=wh)


ROUTES = {
    "plain": lambda b: msda.ms_deform_attn(b["value"], b["shapes"], b["start"], b["loc"], b["weights"]),
    "fused": lambda b: msda.ms_deform_attn_fused(b["value"], b["shapes"], b["start"], b["offsets"], b["logits"], b["ref"]),
    "ATen + plain": lambda b: msda.ms_deform_attn(b["value"], b["shapes"], b["start"],
                                                  *aten_prep(b["offsets"], b["logits"], b["ref"], b["wh"])),
    "grid_sample": lambda b: grid_sample_route(b["value"], b["loc"], b["weights"]),
}


def capture(route, blocks, per_graph):
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
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


def main():
    print("%s, torch %s; graphs of back-to-back calls, %d replays per figure, %d rounds, routes alternating"
          % (torch.cuda.get_device_name(0), torch.__version__, REPLAYS, ROUNDS))
    print("N=%d levels %s S=Lq=%d M=%d D=%d P=%d" % (N, ", ".join("%dx%d" % s for s in LEVELS), S, M, D, P))
    with torch.no_grad():
        shapes = torch.tensor(LEVELS, dtype=torch.int64, device=DEV)
        start = torch.tensor([0, LEVELS[0][0] * LEVELS[0][1], LEVELS[0][0] * LEVELS[0][1] + LEVELS[1][0] * LEVELS[1][1]],
                             dtype=torch.int64, device=DEV)
        wh = shapes.flip(-1)
        blocks = [make_block(100 + k, shapes, start, wh) for k in range(BLOCKS)]
        b0 = blocks[0]
        outs = {name: fn(b0) for name, fn in ROUTES.items()}  # (also the warm-up of every route)
        torch.cuda.synchronize()
        rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
        print("agreement on block 0 (L2 relative): plain vs grid_sample %.2e, fused vs ATen + plain %.2e, ATen + plain vs plain %.2e"
              % (rel(outs["plain"], outs["grid_sample"]), rel(outs["fused"], outs["ATen + plain"]),
                 rel(outs["ATen + plain"], outs["plain"])))
        assert rel(outs["plain"], outs["grid_sample"]) < 1e-5 and rel(outs["fused"], outs["plain"]) < 1e-5
        outside = float(((b0["loc"] < 0) | (b0["loc"] > 1)).any(-1).float().mean())
        print("%.1f %% of the samples outside [0,1]" % (100 * outside))
        nbytes = 4 * (b0["value"].numel() + b0["loc"].numel() + b0["weights"].numel() + outs["plain"].numel())
        floor_us = nbytes / PEAK * 1e6
        print("byte floor: %.1f MB (value + locations + weights + output) / 8 TB/s = %.1f us" % (nbytes / 1e6, floor_us))
        for regime, use in (("cold (8 argument blocks in rotation)", blocks), ("warm (one argument block)", blocks[:1])):
            per = {name: (PER_GRAPH if "grid" not in name and "ATen" not in name else 8) for name in ROUTES}
            graphs = {name: capture(name, use, per[name]) for name in ROUTES}
            times = {name: [] for name in ROUTES}
            for _ in range(ROUNDS):
                for name in ROUTES:
                    times[name].append(replay_us(graphs[name], per[name]))
            med = {name: statistics.median(t) for name, t in times.items()}
            print(regime)
            for name in ROUTES:
                t = times[name]
                line = "   %-14s %9.1f us   (%.1f .. %.1f)" % (name, med[name], min(t), max(t))
                if name in ("plain", "fused"):
                    line += "   x%.1f against grid_sample, %.1f x the byte floor (%.2f TB/s algorithmic)" % (
                        med["grid_sample"] / med[name], med[name] / floor_us, nbytes / med[name] / 1e6)
                print(line)
            print("   fused against ATen + plain: x%.2f" % (med["ATen + plain"] / med["fused"]))
            del graphs


if __name__ == "__main__":
    t = time.perf_counter()
    main()
    print("(%.1f s)" % (time.perf_counter() - t))
