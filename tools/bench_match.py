#!/usr/bin/env python3
"""Matching consecutive frames of a device-resident batch on one MI355X (not
the bench.py metric).

The bench's 128 synthetic 1920x1080 frames are extracted once with the
results left in HBM (sift_batch_device(..., fetch=False)); the 127 pairs
(i, i + 1) are then matched three ways, in this one process:

  (a) match_frames on the device results: cross-check + ratio 0.8, one call
      (sift_mi_match_pairs_device);
  (b) the route without it: copy the descriptors to the host (the cheapest
      fetch there is: one device-to-host copy of the descriptor arena), slice
      them per frame and call match_descriptors (cross-check; it has no ratio
      test) once per pair;
  (c) the kernels of (a) alone, from the HIP events the library records
      around them (stats()["match_ms"]), and their share of the bf16 MFMA
      peak (2.5 PFLOP/s dense) counting 2 * 128 flop per (query, train) row
      pair of the matched segments.

With ratio off (a) must return exactly (b)'s matches: checked for every pair.
Each GPU step runs under its own time limit (SIGALRM); one that runs out ends
the tool at once with a non-zero status (a call that never returns from the
library is not interrupted: run the tool itself under `timeout` as well).
Prints one JSON line; exits non-zero unless (a) is faster than (b).
    python tools/bench_match.py [--frames 128] [--steps 3] [--ratio 0.8]
"""
import argparse
import contextlib
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sift-features_amd"))

BF16_PEAK_FLOPS = 2.5e15


@contextlib.contextmanager
def limit(seconds, what):
    def on_alarm(signum, frame):
        raise TimeoutError(f"{what}: no result within {seconds} s")
    old = signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--ratio", type=float, default=0.8)
    a = ap.parse_args()
    import torch
    import pkg_loader
    import shard
    import synth
    pkg = pkg_loader.load()
    n, W, H = a.frames, a.width, a.height
    pairs = [(i, i + 1) for i in range(n - 1)]

    with limit(120, "frames + extraction"):
        fr = synth.frames_torch(n, W, H, seed0=0, device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        ctx = pkg.Context(0, pkg.OpenCVProcessing)
        offs, _ = ctx.sift_batch_device(fr.data_ptr(), n, W, H, fr.stride(1), fr.stride(0), fetch=False)
    counts = np.diff(offs)
    pair_rows = float(sum(int(counts[i]) * int(counts[j]) for i, j in pairs))

    # (a) and (c)
    with limit(120, "match_frames warm-up"):
        got = ctx.match_frames(offs, pairs, ratio=a.ratio, cross_check=True)  # grows the scratch
    ts = []
    ctx.reset_stats()
    with limit(120, "match_frames"):
        for _ in range(a.steps):
            t0 = time.perf_counter()
            got = ctx.match_frames(offs, pairs, ratio=a.ratio, cross_check=True)
            ts.append(time.perf_counter() - t0)
    st = ctx.stats()
    a_ms = 1e3 * float(np.median(ts))
    c_ms = st["match_ms"] / a.steps
    n_ratio = sum(len(g[0]) for g in got)

    # (b): a second context does the host-array calls, so the device results stay untouched
    mctx = pkg.Context(0, pkg.OpenCVProcessing)

    def host_route():
        _, d = shard.device_results(ctx)
        host = d.cpu().numpy()
        return [mctx.match_descriptors(host[offs[i]:offs[i + 1]], host[offs[j]:offs[j + 1]], cross_check=True)
                for i, j in pairs]

    with limit(300, "host route warm-up"):
        ref = host_route()
    tb = []
    with limit(600, "host route"):
        for _ in range(a.steps):
            t0 = time.perf_counter()
            ref = host_route()
            tb.append(time.perf_counter() - t0)
    b_ms = 1e3 * float(np.median(tb))

    # ratio off: (a) is exactly (b)
    with limit(120, "match_frames, ratio off"):
        plain = ctx.match_frames(offs, pairs, cross_check=True)
    same = all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and
               np.array_equal(x[2].view(np.uint32), y[2].view(np.uint32)) for x, y in zip(plain, ref))
    print(json.dumps({
        "what": "consecutive-frame matching of a device-resident batch",
        "frames": n, "frame": f"{W}x{H}", "pairs": len(pairs), "keypoints": int(offs[-1]),
        "ratio": a.ratio, "steps": a.steps,
        "a_match_frames_ms": a_ms, "a_all_ms": [1e3 * t for t in ts],
        "b_fetch_then_match_descriptors_ms": b_ms, "b_all_ms": [1e3 * t for t in tb],
        "b_over_a": b_ms / a_ms,
        "c_kernels_ms": c_ms, "c_tiles": int(st["match_tiles"] // a.steps),
        "c_tflops": 2 * 128 * pair_rows / (c_ms * 1e-3) / 1e12,
        "c_share_of_bf16_peak": 2 * 128 * pair_rows / (c_ms * 1e-3) / BF16_PEAK_FLOPS,
        "matches_cross_ratio": n_ratio, "matches_cross": sum(len(g[0]) for g in plain),
        "ratio_off_equals_host_route": bool(same)}))
    mctx.close()
    ctx.close()
    return 0 if same and a_ms < b_ms else 1


if __name__ == "__main__":
    sys.exit(main())
