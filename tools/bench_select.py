#!/usr/bin/env python3
"""Spread-limited selection (adaptive non-maximal suppression) over a
device-resident batch on one MI355X (not the bench.py metric).  LABELLED
EXTENSION: the crate has nothing like it.

128 synthetic 1920x1080 frames: four scenes (synth seeds 0..3) of 32 frames
each, frame i of a scene shifted by (3 i, 2 i) px with wrap-around (a panning
camera), in order, so the 127 consecutive pairs overlap but for the three
scene changes.  They are extracted once with the results left in HBM
(sift_batch_device(..., fetch=False)).

In this one process, after a warm-up call, median over --steps calls:
  select_ms         Context.select_frames (the call: its table upload, the
                    three kernels, the download of rows and radius2)
  kernel_ms         the two events around its launch sequence
                    (sift_mi_select_counters); pair_tests_per_s from it and the
                    counter's pair tests, and f32_flops_share_of_peak: five f32
                    operations a pair test (two differences, two products, one
                    sum; the comparison, the select and the minimum not
                    counted) against the 157.3 TFLOPS vector peak, which
                    counts an fma as two and so is out of reach by a factor of
                    two for a product that must not be fused
  baseline_ms       what a caller has without this call: the keypoints copied
                    to the host (baseline_copy_ms) and tests/select_ref.py's
                    numpy O(n^2) on --baseline-frames frames, scaled to the
                    batch by the pair tests (EXTRAPOLATED, not a measurement);
                    its rows and radii must equal the GPU's on those frames
Downstream, the 127 consecutive pairs through match_pairs_device (ratio 0.8,
cross check) and verify_pairs_device (homography) on three arenas: the
selected one, the full one, and a second extraction with
features_limit = --limit (the cap by response that exists without this call).
For each: wall times, the kernels' share where a counter exists, inliers per
pair and the occupied cells (16 x 16 over the frame) of the kept keypoints per
frame and of the inlier keypoints per pair.
Each GPU step runs under its own time limit (SIGALRM); run the tool itself
under `timeout` as well.  Prints one JSON line; exits non-zero unless the
baseline frames agree.
    python tools/bench_select.py [--scenes 4] [--per-scene 32] [--steps 5] [--limit 2000] [--c 0.9]
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

PEAK_F32_VECTOR_TFLOPS = 157.3


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
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--per-scene", type=int, default=32)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=2000)
    ap.add_argument("--c", type=float, default=0.9)
    ap.add_argument("--ratio", type=float, default=0.8)
    ap.add_argument("--baseline-frames", type=int, default=4)
    a = ap.parse_args()
    import torch
    import pkg_loader
    import select_ref as R
    import shard
    import synth
    pkg = pkg_loader.load()
    n, W, H = a.scenes * a.per_scene, a.width, a.height
    pairs = [(i, i + 1) for i in range(n - 1)]

    def extract(ctx, fr, features_limit=None):
        offs, _ = ctx.sift_batch_device(fr.data_ptr(), n, W, H, fr.stride(1), fr.stride(0),
                                        features_limit=features_limit, fetch=False)
        return np.asarray(offs, np.int64)

    with limit(300, "frames + extraction"):
        dev = torch.device("cuda", 0)
        bases = synth.frames_torch(a.scenes, W, H, seed0=0, device=dev)
        fr = torch.stack([torch.roll(bases[f // a.per_scene], (2 * (f % a.per_scene), 3 * (f % a.per_scene)),
                                     dims=(0, 1)) for f in range(n)]).contiguous()
        torch.cuda.synchronize()
        ctx = pkg.Context(0, pkg.OpenCVProcessing)
        offs = extract(ctx, fr)

    with limit(120, "select_frames"):
        sel = ctx.select_frames(offs, a.limit, a.c)  # grows the scratch
        ctx.reset_stats()
        wall, kern = [], []
        for _ in range(a.steps):
            k0 = ctx.select_counters()["kernel_ms"]
            t0 = time.perf_counter()
            sel = ctx.select_frames(offs, a.limit, a.c)
            wall.append(1e3 * (time.perf_counter() - t0))
            kern.append(ctx.select_counters()["kernel_ms"] - k0)
        tests = ctx.select_counters()["pair_tests"] // a.steps

    # baseline: the keypoints on the host, the restatement on a few frames
    t_kps, _ = shard.device_results(ctx)
    with limit(300, "baseline"):
        t0 = time.perf_counter()
        kps = t_kps.cpu().numpy()
        copy_ms = 1e3 * (time.perf_counter() - t0)
        nb = min(a.baseline_frames, n)
        t0 = time.perf_counter()
        b_sel, b_rows, b_r2 = R.run(kps, offs[:nb + 1], a.limit, a.c)
        base_part_ms = 1e3 * (time.perf_counter() - t0)
        part_tests = int((np.diff(offs[:nb + 1]) ** 2).sum())
        same = bool(np.array_equal(b_sel, sel.offsets[:nb + 1]) and np.array_equal(b_rows, sel.rows[:b_sel[-1]])
                    and np.array_equal(b_r2.view(np.uint32), sel.radius2[:offs[nb] - offs[0]].view(np.uint32)))

    def cells(k):
        return R.occupied_cells(k, W, H)

    def downstream(what, d_kps, d_desc, o, host_kps):
        """Matching and verification of the consecutive pairs on one arena; host_kps[s]: segment s's keypoints."""
        with limit(300, what):
            out = {}
            for rep in range(2):  # the first pass grows the scratch
                m0 = ctx.stats()["match_ms"]
                t0 = time.perf_counter()
                matches = ctx.match_pairs_device(d_desc, o, pairs, ratio=a.ratio, cross_check=True)
                t1 = time.perf_counter()
                ver = ctx.verify_pairs_device(d_kps, o, pairs, matches)
                t2 = time.perf_counter()
                out = {"match_ms": 1e3 * (t1 - t0), "match_kernel_ms": ctx.stats()["match_ms"] - m0,
                       "verify_ms": 1e3 * (t2 - t1)}
            inl = [int(v[2]["n_inliers"]) for v in ver]
            inl_cells = [cells(host_kps[q][m[0][v[1]]]) for (q, _), m, v in zip(pairs, matches, ver)]
            out.update({"keypoints": int(o[-1] - o[0]), "matches_median": float(np.median([len(m[0]) for m in matches])),
                        "inliers_median": float(np.median(inl)), "inliers_min": int(min(inl)),
                        "inliers_sum": int(sum(inl)),
                        "kept_cells_median": float(np.median([cells(k) for k in host_kps])),
                        "inlier_cells_median": float(np.median(inl_cells))})
            return out

    seg = [kps[offs[s]:offs[s + 1]] for s in range(n)]
    d_kps, d_desc, _ = ctx.device_results()
    res_sel = downstream("selected arena", sel.d_kps_ptr, sel.d_desc_ptr, sel.offsets,
                         [seg[s][sel.segment_rows(s)] for s in range(n)])
    res_full = downstream("full arena", d_kps, d_desc, offs, seg)
    with limit(300, "extraction with a features_limit"):
        offs_l = extract(ctx, fr, features_limit=a.limit)
        kps_l = shard.device_results(ctx)[0].cpu().numpy()
        d_kps, d_desc, _ = ctx.device_results()
    res_lim = downstream("features_limit arena", d_kps, d_desc, offs_l, [kps_l[offs_l[s]:offs_l[s + 1]] for s in range(n)])

    k_ms = float(np.median(kern))
    per_s = tests / (k_ms * 1e-3)
    print(json.dumps({
        "what": "spread-limited selection (adaptive non-maximal suppression) over a device-resident batch",
        "frames": n, "frame": f"{W}x{H}", "scenes": a.scenes, "keypoints": int(offs[-1]),
        "keypoints_per_frame_median": float(np.median(np.diff(offs))), "limit": a.limit, "c": a.c, "steps": a.steps,
        "kept": int(sel.offsets[-1]), "infinite_radii": int(np.isinf(sel.radius2).sum()),
        "select_ms": float(np.median(wall)), "all_select_ms": wall, "kernel_ms": k_ms, "all_kernel_ms": kern,
        "pair_tests": int(tests), "pair_tests_per_s": per_s,
        "f32_flops_share_of_peak": 5 * per_s / (PEAK_F32_VECTOR_TFLOPS * 1e12),
        "baseline_copy_ms": copy_ms, "baseline_frames": nb, "baseline_frames_ms": base_part_ms,
        "baseline_ms_EXTRAPOLATED": copy_ms + base_part_ms * tests / max(part_tests, 1),
        "baseline_same_result": same,
        "selected": res_sel, "full": res_full, "features_limit": res_lim}))
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
