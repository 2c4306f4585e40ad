"""DynamicDepth's forward warp (mal_amd/rigid_warp.py) at that trainer's shape on one MI355X:

    python scripts/bench_fwarp.py [calls per graph]      # prints; profiles/fwarp_bench.txt is a copy of the output

B = 12, 192x512, C = 3, upscale 3 (10.6 M sub-points per pose), the two poses of a training step (trainer.py:502,525).  Two
routes, on the same box, inputs and process:

    hip      ONE mal_forward_warp call for both poses: z-buffer clear, prep, splat (integer atomicMax), resolve
    torch    the restatement's torch operators on the device, once per pose: nearest upsampling, three bmm, the divisions,
             truncation, scatter_reduce(amax) for the z-buffer, then the inverse warp with F.grid_sample.  The reference
             itself cannot run there (torch_sparse).  Its three matrix inversions and the Euler round trip are NOT in the
             timed graph (torch.inverse is not capturable): they are precomputed, which favours this route.

Each is measured as scripts/msda_bench.py measures: ONE captured graph of back-to-back calls, call i on argument block
i mod BLOCKS, replayed between two events outside the graph.  Cold: 8 distinct argument blocks; warm: one.  Median and
spread of ROUNDS such measurements, the routes alternating.
Byte floor: depth read once; per pose the z-buffer written by the clear, updated and read (3 x 4 B per cell), the image
gathered once (C x 4 B), three outputs (C + 2) x 4 B; over the 8 TB/s peak."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from mal_amd import ops

DEV = torch.device("cuda:0")
PER_GRAPH = max(int(sys.argv[1]) if len(sys.argv) > 1 else 16, 8)
REPLAYS, ROUNDS, BLOCKS, PEAK = 5, 7, 8, 8.0e12
B, C, H, W, UP, P = 12, 3, 192, 512, 3, 2


def euler_to_mat(a):
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    zero, one = z * 0, z * 0 + 1
    rz = torch.stack([z.cos(), -z.sin(), zero, z.sin(), z.cos(), zero, zero, zero, one], 1).reshape(-1, 3, 3)
    ry = torch.stack([y.cos(), zero, y.sin(), zero, one, zero, -y.sin(), zero, y.cos()], 1).reshape(-1, 3, 3)
    rx = torch.stack([one, zero, zero, zero, x.cos(), -x.sin(), zero, x.sin(), x.cos()], 1).reshape(-1, 3, 3)
    return rx @ ry @ rz


def mat_to_euler(R):
    sy = torch.sqrt(R[:, 0, 0] ** 2 + R[:, 1, 0] ** 2)  # (never singular for these poses)
    return torch.stack([torch.atan2(R[:, 2, 1], R[:, 2, 2]), torch.atan2(-R[:, 2, 0], sy), torch.atan2(R[:, 1, 0], R[:, 0, 0])], -1)


def grid(h, w):
    i = torch.arange(h, device=DEV, dtype=torch.float32).view(1, h, 1).expand(1, h, w)
    j = torch.arange(w, device=DEV, dtype=torch.float32).view(1, 1, w).expand(1, h, w)
    return torch.stack((j, i, torch.ones(1, h, w, device=DEV)), 1).expand(B, 3, h, w).reshape(B, 3, -1)


def make_block(seed):
    """a smooth scene (inverse depth bilinear from an 7x17 random grid, depths 2..50 m), poses of a few centimetres and
    hundredths of a radian"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    disp = 0.02 + 0.48 * F.interpolate(torch.rand(B, 1, 7, 17, device=DEV, generator=g), size=(H, W), mode="bilinear", align_corners=True)
    K = torch.tensor([[0.58 * W, 0, 0.5 * W], [0, 1.92 * H, 0.5 * H], [0, 0, 1]], device=DEV).repeat(B, 1, 1)
    poses = []
    for _ in range(P):
        ang = 0.01 * torch.randn(B, 3, device=DEV, generator=g)
        t = 0.05 * torch.randn(B, 3, 1, device=DEV, generator=g)
        poses.append(torch.cat([euler_to_mat(ang), t], 2).contiguous())
    blk = dict(img=torch.rand(B, C, H, W, device=DEV, generator=g), depth=(1 / disp)[:, 0].contiguous(), K=K, poses=poses)
    # what the torch route is handed for free: the inverses and the Euler round trip
    K_u = torch.cat((K[:, :2] * UP, K[:, 2:]), 1)
    blk["Kiu"], blk["Ki"] = K_u.inverse(), K.inverse()
    last = torch.tensor([0.0, 0, 0, 1], device=DEV).view(1, 1, 4).repeat(B, 1, 1)
    blk["proj"] = []
    for p in poses:
        inv = torch.inverse(torch.cat([p, last], 1))
        blk["proj"].append(K @ torch.cat([euler_to_mat(mat_to_euler(inv[:, :3, :3])), inv[:, :3, 3:]], 2))
    blk["grid_u"], blk["grid"] = grid(H * UP, W * UP), grid(H, W)
    return blk


def torch_route(b, stats=None):
    outs = []
    for p, proj in zip(b["poses"], b["proj"]):
        depth_u = F.interpolate(b["depth"].unsqueeze(1), scale_factor=UP).reshape(B, 1, -1)
        cam = (b["Kiu"] @ b["grid_u"]) * depth_u
        m = p[:, :, :3] @ cam + p[:, :, 3:]
        Z = m[:, 2].clamp(min=1e-3)
        pix = b["K"] @ torch.stack([m[:, 0] / Z, m[:, 1] / Z, Z / Z], 1)
        x, y = pix[:, 0], pix[:, 1]
        inside = (x > -1) & (x < W) & (y > -1) & (y < H)
        cell = torch.where(inside, torch.where(inside, y, 0).long() * W + torch.where(inside, x, 0).long(), H * W)
        zbuf = torch.zeros(B, H * W + 1, device=DEV).scatter_reduce(1, cell, 1 / Z, "amax", include_self=True)[:, :-1]
        if stats is not None:  # sub-points inside, and distinct (sample, source pixel, cell) triples
            src = (torch.arange(H * UP, device=DEV).view(-1, 1) // UP * W + torch.arange(W * UP, device=DEV).view(1, -1) // UP).reshape(1, -1)
            key = ((torch.arange(B, device=DEV).view(-1, 1) * (H * W) + src) * (H * W + 1) + cell)[inside]
            stats.append((int(inside.sum()), int(torch.unique(key).numel())))
        fw = zbuf != 0
        depth_w = torch.where(fw, 1 / zbuf, 0)
        cam2 = (b["Ki"] @ b["grid"]) * depth_w.unsqueeze(1)
        q = proj[:, :, :3] @ cam2 + proj[:, :, 3:]
        Z2 = q[:, 2].clamp(min=1e-3)
        coords = torch.stack([2 * (q[:, 0] / Z2) / (W - 1) - 1, 2 * (q[:, 1] / Z2) / (H - 1) - 1], 2).reshape(B, H, W, 2)
        img_s = F.grid_sample(b["img"], coords, padding_mode="zeros", align_corners=True)
        valid = (fw.reshape(B, H, W) & (coords.abs().max(-1)[0] <= 1)).float().unsqueeze(1)
        outs.append((img_s * valid, depth_w.reshape(B, 1, H, W) * valid, valid, zbuf.reshape(B, H, W)))
    return outs


ROUTES = {
    "hip": lambda b: ops.forward_warp(b["img"], b["depth"], b["poses"], b["K"], UP),
    "torch": torch_route,
}


def capture(route, blocks, per_graph):
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for b in blocks[:1]:
            ROUTES[route](b)  # the workspace of this stream, outside the capture
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


def agreement(b0):
    hip = ops.forward_warp(b0["img"], b0["depth"], b0["poses"], b0["K"], UP, want_zbuf=True)
    stats = []
    ref = torch_route(b0, stats)
    for q in range(P):
        z = hip[3][q].view(torch.float32)
        same = (z - ref[q][3]).abs() <= 2e-6 * ref[q][3]  # (the torch route's bmm rounds in its own order)
        v_same = hip[2][q] == ref[q][2][:, 0]
        both = (same & v_same).unsqueeze(1)
        d_img = float(((hip[0][q] - ref[q][0]).abs() * both).max())
        print("pose %d: z-buffer cells within 2e-6 of the torch route's %.4f %%, holes %.1f %%, valid equal %.4f %%, img_w max |diff| %.2e where both are"
              % (q, 100 * float(same.float().mean()), 100 * float((z == 0).float().mean()), 100 * float(v_same.float().mean()), d_img))
        assert float(same.float().mean()) > 0.999 and float(v_same.float().mean()) > 0.999 and d_img < 1e-3
    inside = sum(s[0] for s in stats)
    pairs = sum(s[1] for s in stats)
    print("sub-points per call %.2f M, inside %.2f M, distinct (source pixel, cell) pairs %.2f M = the global atomics a complete "
          "in-register merge issues (%.2f per source pixel)" % (P * B * H * W * UP * UP / 1e6, inside / 1e6, pairs / 1e6, pairs / (P * B * H * W)))


def main():
    print("%s, torch %s; graphs of back-to-back calls, %d replays per figure, %d rounds, routes alternating"
          % (torch.cuda.get_device_name(0), torch.__version__, REPLAYS, ROUNDS))
    print("B=%d %dx%d C=%d upscale %d, %d poses per call" % (B, H, W, C, UP, P))
    with torch.no_grad():
        blocks = [make_block(300 + k) for k in range(BLOCKS)]
        agreement(blocks[0])
        nbytes = 4 * (B * H * W + P * B * H * W * (3 + C + C + 2))
        floor_us = nbytes / PEAK * 1e6
        print("byte floor: %.1f MB / 8 TB/s = %.1f us" % (nbytes / 1e6, floor_us))
        result = {}
        for regime, use in (("cold (8 argument blocks in rotation)", blocks), ("warm (one argument block)", blocks[:1])):
            per = {"hip": PER_GRAPH, "torch": 8}
            per.update({name: PER_GRAPH for name in ROUTES if name not in per})
            graphs = {name: capture(name, use, per[name]) for name in ROUTES}
            times = {name: [] for name in ROUTES}
            for _ in range(ROUNDS):
                for name in ROUTES:
                    times[name].append(replay_us(graphs[name], per[name]))
            med = {name: statistics.median(t) for name, t in times.items()}
            print(regime)
            for name in ROUTES:
                t = times[name]
                line = "   %-10s %9.1f us   (%.1f .. %.1f)" % (name, med[name], min(t), max(t))
                if name != "torch":
                    line += "   x%.1f against torch, %.1f x the byte floor" % (med["torch"] / med[name], med[name] / floor_us)
                print(line)
            result[regime] = (med, times)
            del graphs
        med, times = result["cold (8 argument blocks in rotation)"]
        spread = max(max(t) - min(t) for t in times.values())
        verdict = "beats" if med["torch"] - med["hip"] > spread else "does NOT beat"
        print("cold: hip %s the torch route by more than the measured spread (%.1f us apart, spread %.1f us)"
              % (verdict, med["torch"] - med["hip"], spread))


if __name__ == "__main__":
    t = time.perf_counter()
    main()
    print("(%.1f s)" % (time.perf_counter() - t))
