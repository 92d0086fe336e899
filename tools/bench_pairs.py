#!/usr/bin/env python3
"""Frame-pair proposal over an unordered device-resident batch on one MI355X
(not the bench.py metric).  LABELLED EXTENSION: the crate has nothing like it.

128 synthetic 1920x1080 frames: four scenes (synth seeds 0..3) of 32 frames
each, frame i of a scene shifted by (3 i, 2 i) px with wrap-around (a panning
camera), the 128 frames shuffled with a fixed seed.  They are extracted once
with the results left in HBM (sift_batch_device(..., fetch=False)).

In this one process, after a warm-up call, median over --steps calls:
  propose_ms        Context.propose_frames (the call, its n^2 score download
                    and the host's proposal step)
  kernel_ms         the two events around its launch sequence
                    (sift_mi_pair_counters): selection + one tile per pair
  baseline1_ms      the same scores from the API without this call: the subset
                    rows found and gathered with torch (a stable descending
                    sort of the size pattern per frame), match_pairs_device on
                    all n (n - 1) ORDERED pairs of the compact arena, matches
                    counted on the host; baseline1_gather_ms and
                    baseline1_match_kernel_ms (sift_mi_stats.match_ms) are its
                    parts.  Its scores must equal propose_frames'.
  baseline2_ms      match_frames (ratio, cross check) on a sample of the
                    n (n - 1) / 2 unordered pairs at full size (every 64th
                    pair of the list, 127 of 8128 by default);
                    baseline2_all_pairs_ms_EXTRAPOLATED scales it by the pair
                    count and is not a measurement.
Also recall and precision of the proposal against the scene membership (a
pair is true when both frames show the same scene), and the score ranges.
Each GPU step runs under its own time limit (SIGALRM); run the tool itself
under `timeout` as well.  Prints one JSON line; exits non-zero unless
baseline 1 gives the same score matrix.
    python tools/bench_pairs.py [--scenes 4] [--per-scene 32] [--steps 5] [--subset 128] [--min-matches 8]
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
    ap.add_argument("--subset", type=int, default=128)
    ap.add_argument("--ratio", type=float, default=0.8)
    ap.add_argument("--min-matches", type=int, default=8)
    ap.add_argument("--max-partners", type=int, default=0)
    ap.add_argument("--sample-stride", type=int, default=64)
    a = ap.parse_args()
    import torch
    import pkg_loader
    import shard
    import synth
    pkg = pkg_loader.load()
    n, W, H, h = a.scenes * a.per_scene, a.width, a.height, a.subset
    order = np.random.default_rng(2013).permutation(n)
    scene = order // a.per_scene  # frame f of the batch shows scene[f]

    with limit(300, "frames + extraction"):
        dev = torch.device("cuda", 0)
        bases = synth.frames_torch(a.scenes, W, H, seed0=0, device=dev)
        shot = [(int(g) // a.per_scene, int(g) % a.per_scene) for g in order]  # (scene, step of the pan)
        fr = torch.stack([torch.roll(bases[sc], (2 * i, 3 * i), dims=(0, 1)) for sc, i in shot]).contiguous()
        torch.cuda.synchronize()
        ctx = pkg.Context(0, pkg.OpenCVProcessing)
        offs, _ = ctx.sift_batch_device(fr.data_ptr(), n, W, H, fr.stride(1), fr.stride(0), fetch=False)
        offs = np.asarray(offs, np.int64)

    kw = dict(subset=h, ratio=a.ratio, min_matches=a.min_matches, max_partners=a.max_partners)
    with limit(120, "propose_frames"):
        pairs, scores = ctx.propose_frames(offs, **kw)  # grows the scratch
        ctx.reset_stats()
        wall, kern = [], []
        for _ in range(a.steps):
            k0 = ctx.pair_counters()["kernel_ms"]
            t0 = time.perf_counter()
            pairs, scores = ctx.propose_frames(offs, **kw)
            wall.append(1e3 * (time.perf_counter() - t0))
            kern.append(ctx.pair_counters()["kernel_ms"] - k0)

    # baseline 1: the same subsets and scores through match_pairs_device
    t_kps, t_desc = shard.device_results(ctx)
    ordered = [(x, y) for x in range(n) for y in range(n) if x != y]

    def baseline1():
        t0 = time.perf_counter()
        key = t_kps[:, 2].contiguous().view(torch.int32)  # non-negative sizes: the i32 order is the u32 order
        rows, lens = [], []
        for f in range(n):
            lo, hi = int(offs[f]), int(offs[f + 1])
            top = torch.sort(key[lo:hi], descending=True, stable=True).indices[:h]
            rows.append(lo + torch.sort(top).values)
            lens.append(len(top))
        sub = t_desc[torch.cat(rows)].contiguous()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        sub_offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        m0 = ctx.stats()["match_ms"]
        got = ctx.match_pairs_device(sub.data_ptr(), sub_offs, ordered, ratio=a.ratio or None, cross_check=True)
        m1 = ctx.stats()["match_ms"]
        sc = np.zeros((n, n), np.uint32)
        for (x, y), m in zip(ordered, got):
            sc[x, y] = len(m[0])
        t2 = time.perf_counter()
        return sc, 1e3 * (t2 - t0), 1e3 * (t1 - t0), m1 - m0

    with limit(300, "baseline 1"):
        baseline1()
        b1 = [baseline1() for _ in range(max(1, min(a.steps, 3)))]
    same = bool(np.array_equal(b1[-1][0], scores))

    # baseline 2: a sample of the all-pairs list at full size
    every = [(x, y) for x in range(n) for y in range(x + 1, n)]
    sample = every[::a.sample_stride]
    with limit(300, "baseline 2"):
        ctx.match_frames(offs, sample, ratio=a.ratio or None, cross_check=True)
        b2, b2k = [], []
        for _ in range(max(1, min(a.steps, 3))):
            m0 = ctx.stats()["match_ms"]
            t0 = time.perf_counter()
            ctx.match_frames(offs, sample, ratio=a.ratio or None, cross_check=True)
            b2.append(1e3 * (time.perf_counter() - t0))
            b2k.append(ctx.stats()["match_ms"] - m0)

    truth = {(x, y) for x, y in every if scene[x] == scene[y]}
    got = set(pairs)
    s = np.maximum(scores, scores.T)
    eq = scene[:, None] == scene[None, :]
    off = ~np.eye(n, dtype=bool)
    b2_ms, b2_kernel = float(np.median(b2)), float(np.median(b2k))
    scale = len(every) / max(len(sample), 1)
    print(json.dumps({
        "what": "frame-pair proposal (preemptive matching) over an unordered device-resident batch",
        "frames": n, "frame": f"{W}x{H}", "scenes": a.scenes, "keypoints": int(offs[-1]),
        "subset": h, "ratio": a.ratio, "min_matches": a.min_matches, "max_partners": a.max_partners, "steps": a.steps,
        "tiles_per_call": n * (n - 1) // 2,
        "propose_ms": float(np.median(wall)), "all_propose_ms": wall, "kernel_ms": float(np.median(kern)),
        "all_kernel_ms": kern,
        "baseline1_ms": float(np.median([b[1] for b in b1])),
        "baseline1_gather_ms": float(np.median([b[2] for b in b1])),
        "baseline1_match_kernel_ms": float(np.median([b[3] for b in b1])), "baseline1_ordered_pairs": len(ordered),
        "baseline1_same_scores": same,
        "baseline2_sample_pairs": len(sample), "baseline2_ms": b2_ms, "baseline2_match_kernel_ms": b2_kernel,
        "baseline2_all_pairs": len(every), "baseline2_all_pairs_ms_EXTRAPOLATED": b2_ms * scale,
        "baseline2_all_pairs_kernel_ms_EXTRAPOLATED": b2_kernel * scale,
        "proposed": len(got), "true_pairs": len(truth),
        "recall": len(got & truth) / max(len(truth), 1), "precision": len(got & truth) / max(len(got), 1),
        "same_scene_score_min_max": [int(s[eq & off].min()), int(s[eq & off].max())],
        "cross_scene_score_min_max": [int(s[~eq].min()), int(s[~eq].max())] if a.scenes > 1 else None}))
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
