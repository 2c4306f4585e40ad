"""DynamicDepth's occlusion-aware cost volume (mal_amd/costvol.py) at that trainer's shape on one MI355X:

    python scripts/bench_dyn_costvol.py [calls per graph]      # prints; profiles/dyn_costvol_bench.txt is a copy of the output,
                                                               # with the rows of the pool formulation that lost (not in the tree)

B = 12, F = 1, C = 64, 48x128, D = 96, lookup images 192x512 with dark rectangles over about 10 % of the image.  Routes, on the
same box, inputs and process:

    manydepth     mal_cost_volume as it stands (costvol.match_features): the mean over frames, no occlusion handling
    off_mean      mal_cost_volume_dyn, set_1 and pool off, cv_min off: the same arithmetic as the row above
    off           the same with cv_min (upstream's default fusion)
    set_1         occluded samples become 1.0
    pool_r1       the pooled fill (LDS tile), radius 1, threshold 0.7 (the paper's setting)
    pool_r2       radius 2, threshold 0.4 (the encoder's defaults)
    torch         the restatement's torch operators on the device, pool r=1: per sample the 96-fold replication, two
                  grid_samples and a max_pool3d.  Its two host reads (aug_mask, the zero pose) are left out: they cannot be
                  captured, which favours this route.

Each is measured as scripts/bench_fwarp.py measures: ONE captured graph of back-to-back calls, call i on argument block i mod
BLOCKS, replayed between two events outside the graph.  Cold: 8 distinct argument blocks; warm: one.  Median and spread of
ROUNDS such measurements, the routes alternating.

One condition: off_mean and off may exceed manydepth by no more than that row's own min..max spread plus 5 % (the same loop;
a larger gap means the shared path was disturbed).  Everything else is recorded."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from mal_amd import costvol

DEV = torch.device("cuda:0")
PER_GRAPH = max(int(sys.argv[1]) if len(sys.argv) > 1 else 16, 8)
REPLAYS, ROUNDS, BLOCKS = 5, 7, 8
B, Fr, C, h, w, D, H, W = 12, 1, 64, 48, 128, 96, 192, 512


def make_block(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.rand(*s, device=DEV, generator=g)
    cur = torch.relu(torch.randn(B, C, h, w, device=DEV, generator=g))
    look = torch.relu(cur.unsqueeze(1) + 0.3 * torch.randn(B, Fr, C, h, w, device=DEV, generator=g))
    K = torch.tensor([[0.58 * w, 0, 0.5 * w, 0], [0, 1.92 * h, 0.5 * h, 0], [0, 0, 1, 0], [0, 0, 0, 1]], device=DEV).repeat(B, 1, 1)
    poses = torch.eye(4, device=DEV).repeat(B, Fr, 1, 1)
    poses[:, :, :3, 3] = 0.2 * (r(B, Fr, 3) - 0.5) + torch.tensor([0.0, 0.0, -0.2], device=DEV)  # mostly forward motion
    images = 0.1 + 0.8 * r(B * Fr, 3, H, W)
    for n in range(B * Fr):  # two rectangles of 0.22 x 0.22 of the image: about 10 % dark
        for _ in range(2):
            y0, x0 = int(r(1) * (H - 42)), int(r(1) * (W - 113))
            images[n, :, y0:y0 + 42, x0:x0 + 113] *= 0.04
    return dict(cur=cur, look=look, poses=poses, K=K, invK=torch.linalg.inv(K), images=images, bins=torch.linspace(0.4, 9.0, D, device=DEV),
                aug=torch.zeros(B, 1, 1, 1, device=DEV))


def dyn(**o):
    return lambda b: costvol.match_features_dynamic(b["cur"], b["look"], b["poses"], b["K"], b["invK"], b["images"], b["bins"],
                                                    aug_mask=b["aug"], **o)


def torch_route(b, r=1, th=0.7):
    dt = torch.float32
    ys, xs = torch.meshgrid(torch.arange(h, device=DEV, dtype=dt), torch.arange(w, device=DEV, dtype=dt), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(h * w, device=DEV)], 0)
    occ = F.interpolate((b["images"].sum(1).unsqueeze(1) < 0.15).float(), [48, 128])
    inner = torch.zeros(D, h, w, device=DEV)
    inner[:, 2:-2, 2:-2] = 1.0
    vols = []
    for i in range(B):
        cost = torch.ones(D, h, w, device=DEV)
        cam = (b["invK"][i, :3, :3] @ pix).unsqueeze(0) * b["bins"].view(D, 1, 1)
        world = torch.cat([cam, torch.ones(D, 1, h * w, device=DEV)], 1)
        for f in range(Fr):
            P = (b["K"][i] @ b["poses"][i, f])[:3]
            c = P.unsqueeze(0) @ world
            uv = (c[:, :2] / (c[:, 2:3] + 1e-7)).view(D, 2, h, w).permute(0, 2, 3, 1)
            grid = torch.stack([(uv[..., 0] / (w - 1) - 0.5) * 2, (uv[..., 1] / (h - 1) - 0.5) * 2], -1)
            warped = F.grid_sample(b["look"][i:i + 1, f].repeat(D, 1, 1, 1), grid, padding_mode="zeros", mode="bilinear", align_corners=True)
            m = F.grid_sample((occ[i] > 0).float().unsqueeze(0).repeat(D, 1, 1, 1), grid, padding_mode="zeros", mode="bilinear",
                              align_corners=True) > th
            m = m.expand_as(warped)
            x = torch.where(m, 0.0, warped)
            x = F.max_pool3d(x.permute(1, 0, 2, 3), 2 * r + 1, stride=1, padding=r).permute(1, 0, 2, 3)
            warped = torch.where(m, x, warped)
            xv, yv = (grid[..., 0] / 2 + 0.5) * (w - 1), (grid[..., 1] / 2 + 0.5) * (h - 1)
            edge = ((xv >= 2.0) * (xv <= w - 2) * (yv >= 2.0) * (yv <= h - 2)).float() * inner
            diffs = torch.abs(warped - b["cur"][i:i + 1]).mean(1) * edge
            cost = torch.minimum(torch.where(diffs == 0, 1.0, diffs), cost)
        cost = torch.where(cost == 1, 0.0, cost)
        missing = (cost == 0).float()
        vols.append((cost * (1 - missing) + cost.max(0)[0].unsqueeze(0) * missing, missing))
    return torch.stack([v[0] for v in vols]), torch.stack([v[1] for v in vols])


ROUTES = {
    "manydepth": lambda b: costvol.match_features(b["cur"], b["look"], b["poses"], b["K"], b["invK"], b["bins"]),
    "off_mean": dyn(cv_min=False),
    "off": dyn(cv_min=True),
    "set_1": dyn(cv_min=True, set_1=True, pool_th=0.7),
    "pool_r1": dyn(cv_min=True, pool=True, pool_r=1, pool_th=0.7),
    "pool_r2": dyn(cv_min=True, pool=True, pool_r=2, pool_th=0.4),
    "torch": torch_route,
}
PER = {"torch": 2}


def capture(route, blocks, per_graph):
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ROUTES[route](blocks[0])
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
    cv, miss = ROUTES["pool_r1"](b0)
    r_cv, r_miss = torch_route(b0)
    plain = ROUTES["off"](b0)[0]
    close = (cv - r_cv).abs() <= 1e-4
    print("pool_r1 against the torch route: %.3f %% of the cells within 1e-4, missing mask equal on %.3f %%; dark pixels %.1f %%, the pool "
          "changes %.1f %% of the cells against cv_min alone"
          % (100 * float(close.float().mean()), 100 * float((miss == r_miss).float().mean()),
             100 * float((b0["images"].sum(1) < 0.15).float().mean()), 100 * float((cv != plain).float().mean())))
    assert float(close.float().mean()) > 0.98
    a, bb = ROUTES["manydepth"](b0), ROUTES["off_mean"](b0)
    assert torch.equal(a[0], bb[0]) and torch.equal(a[1], bb[1])
    print("off_mean equals manydepth bit for bit")


def main():
    print("%s, torch %s; graphs of back-to-back calls, %d replays per figure, %d rounds, routes alternating"
          % (torch.cuda.get_device_name(0), torch.__version__, REPLAYS, ROUNDS))
    print("B=%d F=%d C=%d %dx%d D=%d, lookup images %dx%d" % (B, Fr, C, h, w, D, H, W))
    with torch.no_grad():
        blocks = [make_block(500 + k) for k in range(BLOCKS)]
        agreement(blocks[0])
        result = {}
        for regime, use in (("cold (8 argument blocks in rotation)", blocks), ("warm (one argument block)", blocks[:1])):
            per = {name: PER.get(name, PER_GRAPH) for name in ROUTES}
            graphs = {name: capture(name, use, per[name]) for name in ROUTES}
            times = {name: [] for name in ROUTES}
            for _ in range(ROUNDS):
                for name in ROUTES:
                    times[name].append(replay_us(graphs[name], per[name]))
            med = {name: statistics.median(t) for name, t in times.items()}
            print(regime)
            for name in ROUTES:
                t = times[name]
                print("   %-10s %9.1f us   (%.1f .. %.1f)   x%.1f against torch" % (name, med[name], min(t), max(t), med["torch"] / med[name]))
            result[regime] = (med, times)
            del graphs
        ok = True
        for regime, (med, times) in result.items():
            base = times["manydepth"]
            allowed = med["manydepth"] * 1.05 + (max(base) - min(base))
            for name in ("off_mean", "off"):
                good = med[name] <= allowed
                ok = ok and good
                print("%s: %s %.1f us against manydepth %.1f us (allowed %.1f): %s" % (regime.split(" ")[0], name, med[name], med["manydepth"],
                                                                                    allowed, "within" if good else "EXCEEDS"))
        if not ok:
            raise SystemExit("the options-off path is slower than mal_cost_volume by more than its spread plus 5 %")


if __name__ == "__main__":
    t = time.perf_counter()
    main()
    print("(%.1f s)" % (time.perf_counter() - t))
