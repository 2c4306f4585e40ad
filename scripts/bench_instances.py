"""The segmenter's inference tail (mal_amd/instances.py, mal_instances) against upstream's tail restated with torch
operators (tests/instances_restated.torch_tail: F.interpolate of all Q planes, softmax, top-k, gather, float threshold,
sigmoid, two products and sums per image) on the same box and inputs, in one run:

    python scripts/bench_instances.py [calls]      # prints; profiles/instances_bench.txt is a copy of the output

Q=100, K=8, T=100, 48x160 -> 192x640, for N=2 (the two warped frames of one confident sample) and N=12 (a batch of target
frames).  After a warm-up the two paths ALTERNATE in blocks of `calls / rounds` calls between device events, so that
clocks and neighbours on the box touch both alike; per path the median block and the spread (min .. max) are printed.
Algorithmic bytes = N Q h w 4 read + N T H W written; their share of the 8 TB/s peak uses the time of the library
call without the Python side: outputs and workspace allocated once, the three launches enqueued back to back."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mal_amd.instances import instance_inference
from tests import instances_restated as R

DEV = torch.device("cuda:0")
CALLS = max(int(sys.argv[1]) if len(sys.argv) > 1 else 300, 100)
ROUNDS = 10
PEAK = 8.0e12
Q, K, T, h, w, H, W = 100, 8, 100, 48, 160, 192, 640


def block_us(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls


def main():
    print("%s, torch %s, %d calls per figure in %d alternating blocks" % (torch.cuda.get_device_name(0), torch.__version__, CALLS, ROUNDS))
    print("Q=%d K=%d T=%d, %dx%d -> %dx%d" % (Q, K, T, h, w, H, W))
    for N in (2, 12):
        for kind in ("N(0, 4) mask logits (half of all pixels set, no row of four without one)",
                     "one +-8 ellipse per query (as a segmenter's planes: most rows of four hold no set pixel)"):
            rng = np.random.default_rng(N)
            logits = torch.from_numpy((rng.standard_normal((N, Q, K + 1)) * 2.0).astype(np.float32)).to(DEV)
            if kind.startswith("N(0"):
                planes = (rng.standard_normal((N, Q, h, w)) * 2.0).astype(np.float32)
            else:
                yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
                cy, cx = rng.integers(8, h - 8, (N, Q, 1, 1)), rng.integers(10, w - 10, (N, Q, 1, 1))
                ry, rx = rng.integers(3, 12, (N, Q, 1, 1)), rng.integers(4, 30, (N, Q, 1, 1))
                planes = np.where(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0, 8.0, -8.0).astype(np.float32)
            planes = torch.from_numpy(planes).to(DEV)
            lib_call = lambda: instance_inference(logits, planes, (H, W), topk=T)
            torch_call = lambda: [t["scores"].shape[0] for t in R.torch_tail(logits, planes, H, W, T)]
            mine, theirs = lib_call(), R.torch_tail(logits, planes, H, W, T)
            for n in range(N):  # the two paths select the same pairs and make the same masks
                i = mine[n]["instances"]
                flat = i.query.long() * K + i.pred_classes
                a, b = torch.argsort(flat), torch.argsort(theirs[n]["flat"])
                assert torch.equal(flat[a], theirs[n]["flat"][b])
                assert int((i.pred_masks[a] != theirs[n]["masks"][b].to(torch.uint8)).sum()) <= 1e-5 * T * H * W
            for _ in range(10):
                lib_call(), torch_call()
            torch.cuda.synchronize()
            per = max(CALLS // ROUNDS, 5)
            a, b = [], []
            for _ in range(ROUNDS):
                a.append(block_us(lib_call, per))
                b.append(block_us(torch_call, per))
            kern = kernel_us(logits, planes, N)
            nbytes = N * Q * h * w * 4 + N * T * H * W
            print("N=%d, %s" % (N, kind))
            print("   mal_amd.instances.instance_inference   %9.1f us   (%.1f .. %.1f)" % (statistics.median(a), min(a), max(a)))
            print("   upstream's tail in torch operators     %9.1f us   (%.1f .. %.1f)   x%.1f"
                  % (statistics.median(b), min(b), max(b), statistics.median(b) / statistics.median(a)))
            print("   the three launches alone               %9.1f us   %.1f MB algorithmic -> %.2f TB/s, %.1f %% of the 8 TB/s peak"
                  % (kern, nbytes / 1e6, nbytes / kern / 1e6, 100.0 * nbytes / (kern * 1e-6) / PEAK))


def kernel_us(logits, planes, N):
    """the library call itself, outputs and workspace allocated once: launches only, between device events"""
    import ctypes
    from mal_amd import _lib as L, ops
    lib, p = L.load(), ops._p
    masks = torch.empty((N, T, H, W), dtype=torch.uint8, device=DEV)
    classes = torch.empty((N, T), dtype=torch.int64, device=DEV)
    f32 = torch.empty((3, N, T), dtype=torch.float32, device=DEV)
    i32 = torch.empty(N * T + N, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(lib.mal_instances_workspace_bytes(N, Q, K, h, w, H, W, T)), dtype=torch.uint8, device=DEV)
    a = L.InstancesArgs()
    a.pred_logits, a.pred_masks, a.thing = p(logits), p(planes), None
    a.N, a.Q, a.K, a.h, a.w, a.H, a.W, a.topk = N, Q, K, h, w, H, W, T
    a.count, a.masks, a.scores, a.classes, a.query = p(i32[N * T:]), p(masks), p(f32[0]), p(classes), p(i32)
    a.cls_score, a.mask_score = p(f32[1]), p(f32[2])
    a.ws, a.ws_bytes, a.stream = p(ws), ws.numel(), ops._stream()
    call = lambda: L.check(lib.mal_instances(ctypes.byref(a)), "mal_instances")
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    return statistics.median(block_us(call, max(CALLS // ROUNDS, 5)) for _ in range(ROUNDS))


if __name__ == "__main__":
    t = time.perf_counter()
    main()
    print("(%.1f s)" % (time.perf_counter() - t))
