#!/usr/bin/env python3
"""Verifying the matched consecutive frames of a device-resident batch on one
MI355X (not the bench.py metric).  LABELLED EXTENSION: the crate has no
geometric verification.

The bench's 128 synthetic 1920x1080 frames are extracted once with the
results left in HBM (sift_batch_device(..., fetch=False)) and the 127 pairs
(i, i + 1) matched with match_frames (cross-check, ratio 0.8; --ratio 0 for
the cross-check alone, which leaves about twenty times as many matches).
Then, in this one process:

  (a) verify_frames on the device keypoints at its defaults (threshold 3,
      1024 hypotheses, 2 refit rounds): one synchronous call
      (sift_mi_verify_pairs_device), median wall time after a warm-up;
  (b) the route without it: copy the keypoints to the host (one
      device-to-host copy of the keypoint arena) and run the numpy
      restatement (tests/verify_ref.py) once per pair.

--model fundamental measures the epipolar model instead (verify_epipolar.hip;
the restatement is tests/epipolar_ref.py) and, in the same run, times
verify_frames with model="homography" as its yardstick
("homography_verify_frames_ms").

The synthetic frames are independent, so the matches are wrong ones and the
models meaningless; the cost does not depend on that except in the refit.
Reports how many pairs (a) and (b) agree on (mask and counts): every pair
without refits; with refits a match within rounding of the threshold may
differ on such data.
Each GPU step runs under its own time limit (SIGALRM); run the tool itself
under `timeout` as well.  Prints one JSON line; exits non-zero unless (a) is
faster than (b) and the two agree without refits.
    python tools/bench_verify.py [--frames 128] [--steps 5] [--host-steps 1] [--ratio 0.8]
                                 [--model homography|fundamental]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=1)
    ap.add_argument("--ratio", type=float, default=0.8)
    ap.add_argument("--model", choices=["homography", "fundamental"], default="homography")
    a = ap.parse_args()
    import torch
    import pkg_loader
    import shard
    import synth
    if a.model == "fundamental":
        import epipolar_ref as verify_ref
    else:
        import verify_ref
    pkg = pkg_loader.load()
    n, W, H = a.frames, a.width, a.height
    pairs = [(i, i + 1) for i in range(n - 1)]

    with limit(120, "frames + extraction + matching"):
        fr = synth.frames_torch(n, W, H, seed0=0, device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        ctx = pkg.Context(0, pkg.OpenCVProcessing)
        offs, _ = ctx.sift_batch_device(fr.data_ptr(), n, W, H, fr.stride(1), fr.stride(0), fetch=False)
        matches = ctx.match_frames(offs, pairs, ratio=a.ratio or None, cross_check=True)
    n_matches = sum(len(m[0]) for m in matches)

    # (a)
    with limit(120, "verify_frames warm-up"):
        got = ctx.verify_frames(offs, pairs, matches, model=a.model)  # grows the scratch
    ts = []
    with limit(120, "verify_frames"):
        for _ in range(a.steps):
            t0 = time.perf_counter()
            got = ctx.verify_frames(offs, pairs, matches, model=a.model)
            ts.append(time.perf_counter() - t0)
    a_ms = 1e3 * float(np.median(ts))
    with limit(120, "verify_frames, no refit"):
        t0 = time.perf_counter()
        plain = ctx.verify_frames(offs, pairs, matches, refit_rounds=0, model=a.model)
        plain_ms = 1e3 * (time.perf_counter() - t0)
    yard = {}
    if a.model != "homography":  # the yardstick, in the same run
        th = []
        with limit(120, "verify_frames, homography"):
            ctx.verify_frames(offs, pairs, matches)
            for _ in range(a.steps):
                t0 = time.perf_counter()
                ctx.verify_frames(offs, pairs, matches)
                th.append(time.perf_counter() - t0)
        yard = {"homography_verify_frames_ms": 1e3 * float(np.median(th)), "homography_all_ms": [1e3 * t for t in th]}

    # (b)
    def host_route(rounds):
        kps = shard.device_results(ctx)[0].cpu().numpy()
        return [verify_ref.verify(verify_ref.records(kps[offs[i]:offs[i + 1]], kps[offs[j]:offs[j + 1]], m),
                                  3.0, 1024, 0, rounds) for (i, j), m in zip(pairs, matches)]

    tb = []
    with limit(900, "host route"):
        for _ in range(a.host_steps):
            t0 = time.perf_counter()
            ref = host_route(2)
            tb.append(time.perf_counter() - t0)
    if not tb:  # --host-steps 0: (a) alone, e.g. under a profiler
        print(json.dumps({"model": a.model, "frames": n, "pairs": len(pairs), "ratio": a.ratio, "matches": n_matches,
                          "a_verify_frames_ms": a_ms, "a_all_ms": [1e3 * t for t in ts], "a_no_refit_ms": plain_ms,
                          **yard}))
        ctx.close()
        return 0
    b_ms = 1e3 * float(np.median(tb))
    with limit(900, "host route, no refit"):
        ref0 = host_route(0)

    def agree(x, y):
        return sum(bool(g[2] == r[2] and np.array_equal(g[1], r[1])) for g, r in zip(x, y))

    exact0 = sum(bool(g[2] == r[2] and np.array_equal(g[1], r[1]) and
                      np.array_equal(g[0].view(np.uint32), r[0].view(np.uint32))) for g, r in zip(plain, ref0))
    print(json.dumps({
        "what": f"RANSAC {a.model} + refit of the matched consecutive frames of a device-resident batch",
        "model": a.model,
        "frames": n, "frame": f"{W}x{H}", "pairs": len(pairs), "keypoints": int(offs[-1]),
        "ratio": a.ratio, "matches": n_matches, "steps": a.steps,
        "a_verify_frames_ms": a_ms, "a_all_ms": [1e3 * t for t in ts], "a_no_refit_ms": plain_ms, **yard,
        "b_fetch_then_numpy_ms": b_ms, "b_all_ms": [1e3 * t for t in tb], "b_over_a": b_ms / a_ms,
        "inliers": sum(g[2]["n_inliers"] for g in got), "models": sum(g[2]["best_hypothesis"] >= 0 for g in got),
        "refits": sum(g[2]["refits"] for g in got),
        "pairs_bit_exact_no_refit": exact0, "pairs_agree_with_refit": agree(got, ref)}))
    ctx.close()
    return 0 if exact0 == len(pairs) and a_ms < b_ms else 1


if __name__ == "__main__":
    sys.exit(main())
