"""DynamicDepth's hole-aware reprojection loss (mal_amd/csrc/mal_holes.hip) at that trainer's Cityscapes shape on one MI355X:

    python scripts/bench_dyn_loss.py [calls per graph]      # prints; profiles/dyn_loss_bench.txt is a copy of the output

B = 12, 192x512, one scale, the reprojection term of one teacher ``compute_losses`` and its backward (trainer.py:1025-1090 with
--zero_img and --selec_reproj, the defaults): the warped pair against the target, the identity pair against the target the
warped pair zeroed, the automask, d loss / d warped candidates.  Every source frame carries two dark rectangles.  Three routes
on the same box, inputs and process:

    holes    mal_photo_holes_fwd + mal_holes_commit (warped pair), the same two for the identity pair, mal_holes_weight,
             mal_photo_holes_bwd.  The target is written in place, so from the second call of a graph on it already holds the
             zeros (the kernels' work does not depend on that).
    torch    tests/dyn_loss_restated.photo_holes -- the reference's own operators -- on the device, with autograd's backward
    plain    ops.photo_fwd (identity pair), ops.photo_fwd + ops.photo_bwd (warped pair, automask in the kernel) on the same
             images: ManyDepth's hole-free arithmetic in the library's default (marching) formulation -- what the extra
             semantics cost against

Measured as scripts/bench_fwarp.py measures: ONE captured graph of back-to-back calls, call i on argument block i mod BLOCKS,
replayed between two events outside the graph.  Cold: 8 distinct argument blocks; warm: one.  Median and spread of ROUNDS such
measurements, the routes alternating."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from mal_amd import _lib as L
from mal_amd import ops
from tests import dyn_loss_restated as R

DEV = torch.device("cuda:0")
PER_GRAPH = max(int(sys.argv[1]) if len(sys.argv) > 1 else 16, 8)
REPLAYS, ROUNDS, BLOCKS = 5, 7, 8
B, H, W = 12, 192, 512
FLAGS = L.F_ZERO_IMG | L.F_SELECT


def textured(g):
    low = F.interpolate(torch.rand(B, 3, 12, 32, device=DEV, generator=g), size=(H, W), mode="bilinear", align_corners=True)
    return (0.1 + 0.8 * low + 0.05 * torch.rand(B, 3, H, W, device=DEV, generator=g)).clamp(0.06, 1)


def make_block(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    tgt = textured(g)
    imgs = []
    for k in range(4):   # warped -1, warped +1, identity -1, identity +1: the target plus a perturbation, two dark rectangles each
        im = (tgt + 0.05 * torch.randn(B, 3, H, W, device=DEV, generator=g)).clamp(0.06, 1)
        for _ in range(2):
            y0 = int(torch.randint(0, H - 48, (1,), device=DEV, generator=g))
            x0 = int(torch.randint(0, W - 96, (1,), device=DEV, generator=g))
            im[:, :, y0:y0 + 40, x0:x0 + 80] = 0.0
        imgs.append(im.contiguous())
    return dict(target0=tgt.contiguous(), target=tgt.clone().contiguous(), warped=imgs[:2], ident=imgs[2:],
                noise=torch.randn(B, 1, H, W, device=DEV, generator=g), scale=torch.ones(1, device=DEV))


def holes_route(b):
    t = b["target"]
    seen = t.clone()
    holes, mn, ch, _, _ = ops.photo_holes_fwd(t, b["warped"], None, None, None, FLAGS)
    ops.holes_commit(t, holes)
    ih, idn, _, _, _ = ops.photo_holes_fwd(t, b["ident"], None, None, None, FLAGS & ~L.F_SELECT)
    ops.holes_commit(t, ih)
    wt, sums = ops.holes_weight(mn, idn, b["noise"], None)
    return sums, ops.photo_holes_bwd(seen, b["warped"], holes, ch, wt, b["scale"], sums, FLAGS, [True, True])


def torch_route(b):
    leaves = [x.detach().requires_grad_(True) for x in b["warped"]]
    first = R.photo_holes(b["target0"], leaves, FLAGS, torch.float32)
    ident = R.photo_holes(first["target_after"], b["ident"], FLAGS & ~L.F_SELECT, torch.float32)
    idn = ident["rp"].detach() + b["noise"] * 0.00001
    w = (first["rp"] <= idn).float().detach()
    loss = (first["rp"] * w).sum() / (w.sum() + 1e-7)
    return loss, torch.autograd.grad(loss, leaves)


def plain_route(b):
    idn, _, _, _ = ops.photo_fwd(b["target0"], b["ident"], None, None, None, 0, want_argmin=False, want_weight=False)
    mn, am, wt, sums = ops.photo_fwd(b["target0"], b["warped"], idn, b["noise"], None, L.F_AUTOMASK)
    return sums, ops.photo_bwd(b["target0"], b["warped"], am, wt, b["scale"], sums, 0, [True, True])


ROUTES = {"holes": holes_route, "torch": torch_route, "plain": plain_route}


def capture(route, blocks, per_graph):
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ROUTES[route](blocks[0])  # the workspace of this stream, outside the capture
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


def agreement(b):
    """the routes compute the same thing: holes against torch on a fresh target; the hole share of the data"""
    b["target"].copy_(b["target0"])
    sums, g = holes_route(b)
    loss, gt = torch_route(b)
    torch.cuda.synchronize()
    mine = float(sums[0] / (sums[1] + 1e-7))
    hs = [R.hole_bytes(x) for x in b["warped"] + b["ident"]]
    print("hole share: warped %.1f %%, %.1f %%; identity %.1f %%, %.1f %%; target zeroed after the call %.1f %%"
          % tuple([100 * float(h.float().mean()) for h in hs] + [100 * float((b["target"].sum(1) == 0).float().mean())]))
    # each route takes its own near-tie decisions (argmin, automask): a flipped pixel moves the gradient of its 3x3
    # neighbourhood, so the share of differing elements is compared, not the maximum (tests/test_gpu_dyn_loss.py forces them)
    share = max(float(((a - c).abs() > 1e-3 * float(c.abs().max())).float().mean()) for a, c in zip(g, gt))
    print("loss: holes %.7f, torch %.7f; gradient elements differing by more than 1e-3 of the largest: %.2e of them"
          % (mine, float(loss.detach()), share))
    assert abs(mine - float(loss.detach())) <= 1e-4 * abs(float(loss.detach())) and share < 1e-3


def main():
    print("%s, torch %s; graphs of back-to-back calls, %d replays per figure, %d rounds, routes alternating"
          % (torch.cuda.get_device_name(0), torch.__version__, REPLAYS, ROUNDS))
    print("B=%d %dx%d, one scale: the teacher's reprojection term (warped pair, identity pair, automask) and its backward" % (B, H, W))
    blocks = [make_block(500 + k) for k in range(BLOCKS)]
    agreement(blocks[0])
    result = {}
    for regime, use in (("cold (8 argument blocks in rotation)", blocks), ("warm (one argument block)", blocks[:1])):
        per = {"holes": PER_GRAPH, "plain": PER_GRAPH, "torch": 8}
        graphs = {name: capture(name, use, per[name]) for name in ROUTES}
        times = {name: [] for name in ROUTES}
        for _ in range(ROUNDS):
            for name in ROUTES:
                times[name].append(replay_us(graphs[name], per[name]))
        med = {name: statistics.median(t) for name, t in times.items()}
        print(regime)
        for name in ROUTES:
            t = times[name]
            print("   %-8s %9.1f us   (%.1f .. %.1f)" % (name, med[name], min(t), max(t)))
        print("   holes / torch = %.3f, holes / plain = %.2f" % (med["holes"] / med["torch"], med["holes"] / med["plain"]))
        result[regime] = (med, times)
        del graphs
    med, times = result["cold (8 argument blocks in rotation)"]
    spread = max(max(times[k]) - min(times[k]) for k in ("holes", "torch"))
    verdict = "beats" if med["torch"] - med["holes"] > spread else "does NOT beat"
    print("cold: holes %s the torch route by more than the measured spread (%.1f us apart, spread %.1f us)"
          % (verdict, med["torch"] - med["holes"], spread))


if __name__ == "__main__":
    t = time.perf_counter()
    main()
    print("(%.1f s)" % (time.perf_counter() - t))
