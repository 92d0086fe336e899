#!/usr/bin/env python3
"""Guided re-matching of the verified consecutive frames of a device-resident
batch on one MI355X (not the bench.py metric).  LABELLED EXTENSION: the crate
has no guided matching.

128 synthetic 1920x1080 frames are extracted once with the results left in HBM
(sift_batch_device(..., fetch=False)); the 127 pairs (i, i + 1) are matched
with match_frames (cross-check, ratio 0.8), verified with verify_frames at its
defaults, and matched again under the fitted homographies with
match_frames_guided (cross-check, threshold 3).  --scene pan (default): the
frames are one synthetic frame shifted by (3 i, 2 i) px with wrap-around, a
panning camera, so the pairs have true matches and real models; --scene
independent: bench.py's independent frames, whose matches are wrong ones and
whose pairs mostly end without a model (an empty guided result).

In this one process, each after a warm-up call, median over --steps calls,
wall time of the call and kernel time (the call's match_ms):
  (a) match_frames_guided with the cull on (SIFT_MI_PATH_GUIDED_CULL = 1),
  (b) the same with the cull off,
  (c) the unguided match_frames of the same pairs,
  (d) the numpy restatement (tests/guided_ref.py) on the fetched keypoints and
      descriptors for the first --host-pairs pairs, EXTRAPOLATED to all pairs
      (labelled so in the output).
Also the culled share of the waves, the match counts before and after, and
whether (a), (b) and (d) agree bit for bit.
Each GPU step runs under its own time limit (SIGALRM); run the tool itself
under `timeout` as well.  Prints one JSON line; exits non-zero unless (a) and
(b) agree with each other and with (d).
    python tools/bench_guided.py [--frames 128] [--steps 5] [--host-pairs 1] [--scene pan|independent]
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


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--host-pairs", type=int, default=1)
    ap.add_argument("--scene", choices=["pan", "independent"], default="pan")
    a = ap.parse_args()
    import torch
    import pkg_loader
    import shard
    import synth
    import guided_ref
    pkg = pkg_loader.load()
    n, W, H = a.frames, a.width, a.height
    pairs = [(i, i + 1) for i in range(n - 1)]

    with limit(180, "frames + extraction + matching + verification"):
        dev = torch.device("cuda", 0)
        if a.scene == "pan":
            base = synth.frames_torch(1, W, H, seed0=0, device=dev)[0]
            fr = torch.stack([torch.roll(base, (2 * i, 3 * i), dims=(0, 1)) for i in range(n)]).contiguous()
        else:
            fr = synth.frames_torch(n, W, H, seed0=0, device=dev)
        torch.cuda.synchronize()
        ctx = pkg.Context(0, pkg.OpenCVProcessing)
        offs, _ = ctx.sift_batch_device(fr.data_ptr(), n, W, H, fr.stride(1), fr.stride(0), fetch=False)
        matches = ctx.match_frames(offs, pairs, ratio=0.8, cross_check=True)
        verified = ctx.verify_frames(offs, pairs, matches)

    def timed(what, call):
        """-> (result, median wall ms, median kernel ms, all wall ms) after one warm-up call."""
        with limit(180, what):
            res = call()  # grows the scratch
            wall, kern = [], []
            for _ in range(a.steps):
                k0 = ctx.stats()["match_ms"]
                t0 = time.perf_counter()
                res = call()
                wall.append(1e3 * (time.perf_counter() - t0))
                kern.append(ctx.stats()["match_ms"] - k0)
        return res, float(np.median(wall)), float(np.median(kern)), wall

    out = {}
    results = {}
    for name, cull in (("a_guided_cull_on", 1), ("b_guided_cull_off", 0)):
        ctx.reset_stats()
        with ctx.path_options(guided_cull=cull):
            res, w, k, allw = timed(name, lambda: ctx.match_frames_guided(offs, pairs, verified, threshold=3.0))
        c = ctx.guided_counters()
        results[name] = res
        out[name] = {"call_ms": w, "kernel_ms": k, "all_call_ms": allw, "tiles": c["tiles"] // (a.steps + 1),
                     "culled_wave_share": c["culled_waves"] / max(1, 4 * c["tiles"])}
    _, w, k, allw = timed("c_unguided", lambda: ctx.match_frames(offs, pairs, ratio=0.8, cross_check=True))
    out["c_unguided_match_frames"] = {"call_ms": w, "kernel_ms": k, "all_call_ms": allw}

    on, off = results["a_guided_cull_on"], results["b_guided_cull_off"]
    agree = all(same(x, y) for x, y in zip(on, off))
    host_ok, host_ms = None, None
    if a.host_pairs:
        with limit(900, "host route"):
            kps, desc = shard.device_results(ctx)
            kps, desc = kps.cpu().numpy(), desc.cpu().numpy()
            t0 = time.perf_counter()
            ref = [guided_ref.match(desc[offs[i]:offs[i + 1]], desc[offs[j]:offs[j + 1]], kps[offs[i]:offs[i + 1]],
                                    kps[offs[j]:offs[j + 1]], verified[p][0], 3.0)
                   for p, (i, j) in enumerate(pairs[:a.host_pairs])]
            host_ms = 1e3 * (time.perf_counter() - t0)
        host_ok = all(same(x, y) for x, y in zip(on, ref))
        out["d_numpy_restatement"] = {"pairs_run": a.host_pairs, "ms_for_them": host_ms,
                                      "extrapolated_ms_all_pairs": host_ms * len(pairs) / a.host_pairs,
                                      "bit_exact_with_a": host_ok}
    print(json.dumps({
        "what": "guided re-match of the verified consecutive frames of a device-resident batch (homography, 3 px)",
        "scene": a.scene, "frames": n, "frame": f"{W}x{H}", "pairs": len(pairs), "keypoints": int(offs[-1]),
        "steps": a.steps, **out,
        "cull_on_equals_cull_off": agree,
        "matches_before": sum(len(m[0]) for m in matches), "inliers": sum(v[2]["n_inliers"] for v in verified),
        "models": sum(v[2]["best_hypothesis"] >= 0 for v in verified),
        "matches_guided": sum(len(g[0]) for g in on)}))
    ctx.close()
    return 0 if agree and host_ok is not False else 1


if __name__ == "__main__":
    sys.exit(main())
