#!/usr/bin/env python3
"""Progressive (PROSAC) against uniform sampling in the verification of the
matched consecutive frames of a device-resident batch on one MI355X (not the
bench.py metric).  LABELLED EXTENSION: the crate has no geometric verification.

The bench's 128 synthetic 1920x1080 frames are extracted once with the
results left in HBM (sift_batch_device(..., fetch=False)) and the 127 pairs
(i, i + 1) matched with match_frames twice: the cross-check alone, and with
ratio 0.8.  For each match set and each model (homography, fundamental), in
this one process and at verify_frames' defaults (threshold 3, 1024 hypotheses,
2 refit rounds):

  uniform      verify_frames(...)                          median wall time
  progressive  verify_frames(..., sampling="progressive")  median wall time,
               ranked by the matcher's distances

and the inlier totals under both.  The ranking gather's share of the
progressive call is measured from outside as the median of a third call
sequence: the progressive call on the same matches with 1 hypothesis and no
refit, against the uniform call with 1 hypothesis and no refit; their
difference is what ranking (the quadratic gather, the host's growth table and
its upload) adds, since the other kernels have next to nothing to do there.
A kernel trace of the tool (rocprofv3 --kernel-trace --stats -- python
tools/bench_verify_progressive.py --steps 3) gives the kernels' own times.

The synthetic frames are independent, so the matches are wrong ones and the
models meaningless: the inlier totals say nothing about recall here (the
value test in tests/test_prosac_ref_cpu.py does), only that both samplings
run on the same data.  Checks one pair per configuration against the
restatement without refits (tests/prosac_ref.py), bit for bit.
Each GPU step runs under its own time limit (SIGALRM); run the tool itself
under `timeout` as well.  Prints one JSON line; exits non-zero if a checked
pair differs from the restatement.
    python tools/bench_verify_progressive.py [--frames 128] [--steps 5]
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


def median_ms(fn, steps):
    fn()  # grows the scratch
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import pkg_loader
    import prosac_ref
    import shard
    import synth
    import verify_ref
    pkg = pkg_loader.load()
    n, W, H = a.frames, a.width, a.height
    pairs = [(i, i + 1) for i in range(n - 1)]

    with limit(180, "frames + extraction + matching"):
        fr = synth.frames_torch(n, W, H, seed0=0, device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        ctx = pkg.Context(0, pkg.OpenCVProcessing)
        offs, _ = ctx.sift_batch_device(fr.data_ptr(), n, W, H, fr.stride(1), fr.stride(0), fetch=False)
        sets = {"cross_check": ctx.match_frames(offs, pairs, ratio=None, cross_check=True),
                "ratio_0.8": ctx.match_frames(offs, pairs, ratio=0.8, cross_check=True)}
        kps = shard.device_results(ctx)[0].cpu().numpy()

    rows, ok = [], True
    for name, matches in sets.items():
        sizes = [len(m[0]) for m in matches]
        for model in ("homography", "fundamental"):
            with limit(300, f"{name} {model}"):
                uni_ms, uni = median_ms(lambda: ctx.verify_frames(offs, pairs, matches, model=model), a.steps)
                pro_ms, pro = median_ms(lambda: ctx.verify_frames(offs, pairs, matches, model=model,
                                                                  sampling="progressive"), a.steps)
                uni1_ms, _ = median_ms(lambda: ctx.verify_frames(offs, pairs, matches, iterations=1, refit_rounds=0,
                                                                 model=model), a.steps)
                pro1_ms, _ = median_ms(lambda: ctx.verify_frames(offs, pairs, matches, iterations=1, refit_rounds=0,
                                                                 model=model, sampling="progressive"), a.steps)
                plain = ctx.verify_frames(offs, pairs, matches, refit_rounds=0, model=model, sampling="progressive")
            p = int(np.argmax(sizes))  # the largest pair against the restatement
            i, j = pairs[p]
            rec = verify_ref.records(kps[offs[i]:offs[i + 1]], kps[offs[j]:offs[j + 1]], matches[p])
            want = prosac_ref.verify(rec, matches[p][2], model, 3.0, 1024, 0, 0)
            exact = bool(plain[p][2] == want[2] and np.array_equal(plain[p][1], want[1]) and
                         np.array_equal(plain[p][0].view(np.uint32), want[0].view(np.uint32)))
            ok = ok and exact
            rows.append({"matches_of": name, "model": model, "matches": int(sum(sizes)), "largest_pair": int(max(sizes)),
                         "sum_m2": int(sum(s * s for s in sizes)),
                         "uniform_ms": uni_ms, "progressive_ms": pro_ms, "progressive_over_uniform": pro_ms / uni_ms,
                         "ranking_added_ms": pro1_ms - uni1_ms, "uniform_1_hypothesis_ms": uni1_ms,
                         "progressive_1_hypothesis_ms": pro1_ms,
                         "ranking_share_of_progressive": (pro1_ms - uni1_ms) / pro_ms,
                         "inliers_uniform": int(sum(g[2]["n_inliers"] for g in uni)),
                         "inliers_progressive": int(sum(g[2]["n_inliers"] for g in pro)),
                         "models_uniform": int(sum(g[2]["best_hypothesis"] >= 0 for g in uni)),
                         "models_progressive": int(sum(g[2]["best_hypothesis"] >= 0 for g in pro)),
                         "largest_pair_bit_exact_no_refit": exact})
    print(json.dumps({"what": "progressive against uniform sampling, verify_frames on the matched consecutive frames "
                              "of a device-resident batch", "frames": n, "frame": f"{W}x{H}", "pairs": len(pairs),
                      "keypoints": int(offs[-1]), "steps": a.steps, "rows": rows}))
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
