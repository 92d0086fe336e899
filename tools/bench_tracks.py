#!/usr/bin/env python3
"""Feature tracks over the verified matches of a device-resident batch on one
MI355X (not the bench.py metric).  LABELLED EXTENSION: the crate has no
tracks.

128 synthetic 1920x1080 frames, one frame shifted by (3 i, 2 i) px with
wrap-around (a panning camera), are extracted once with the results left in
HBM (sift_batch_device(..., fetch=False)); the 127 pairs (i, i + 1) and the
126 pairs (i, i + 2), so that components close loops, are matched with
match_frames (cross-check, ratio 0.8) and verified with verify_frames at its
defaults; the inlier masks are the tracks' keep masks.

In this one process, after a warm-up call, median over --steps calls:
  call_ms      sift_mi_build_tracks_device alone (its arguments prepared once)
  kernel_ms    the two events around its launch sequence (sift_mi_track_counters)
  upload_ms    the matches (12 bytes each) and the mask (1 byte each) from
               pageable host memory to the device, measured on their own with
               a torch copy of the same size
  download_ms  track_of, track_offsets, conflict and obs to pageable host
               memory, the same way
  check_ms     the host's checks of the offsets, pairs and every match index,
               timed directly: the same call with the LAST match's index set
               to -1 walks all of them and returns SIFT_MI_EINVAL before any
               device work
  rest_ms      call_ms - kernel_ms - upload_ms - download_ms - check_ms: the
               mask count, the tables, the sort's temporary-size query, the
               launches and the two synchronises
  python_ms    Context.track_frames (the call plus its numpy packing)
Also the number of tracks, their length histogram, the share in conflict, the
time of the numpy restatement (tests/tracks_ref.py) on the same data, whether
it agrees bit for bit, and the time of a plain single-thread C++ union-find
over the same edges (tools/bench_tracks_uf.cpp, built here with g++ -O2;
components only: no grouping, no observations).
Each GPU step runs under its own time limit (SIGALRM); run the tool itself
under `timeout` as well.  Prints one JSON line; exits non-zero unless the GPU
result equals the restatement's.
    python tools/bench_tracks.py [--frames 128] [--steps 5] [--min-length 2] [--conflicts flag|drop]
"""
import argparse
import contextlib
import ctypes
import json
import os
import shutil
import signal
import subprocess
import sys
import tempfile
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


def union_find_baseline(n, a, b):
    """ms of tools/bench_tracks_uf.cpp on the edges, None without g++."""
    gxx = shutil.which("g++")
    if not gxx:
        return None
    with tempfile.TemporaryDirectory() as tmp:
        exe, data = os.path.join(tmp, "uf"), os.path.join(tmp, "edges.bin")
        subprocess.check_call([gxx, "-O2", "-std=c++17", os.path.join(ROOT, "tools", "bench_tracks_uf.cpp"), "-o", exe])
        with open(data, "wb") as f:
            np.array([n, len(a)], np.uint32).tofile(f)
            np.stack([a, b], 1).astype(np.uint32).tofile(f)
        runs = [float(subprocess.run([exe, data], capture_output=True, text=True, check=True).stdout.split()[1])
                for _ in range(3)]
    return float(np.median(runs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--min-length", type=int, default=2)
    ap.add_argument("--conflicts", choices=["flag", "drop"], default="flag")
    a = ap.parse_args()
    import torch
    import pkg_loader
    import shard
    import synth
    import tracks_ref as T
    pkg = pkg_loader.load()
    from sift_features_amd import _lib
    n, W, H = a.frames, a.width, a.height
    pairs = [(i, i + 1) for i in range(n - 1)] + [(i, i + 2) for i in range(n - 2)]

    with limit(300, "frames + extraction + matching + verification"):
        dev = torch.device("cuda", 0)
        base = synth.frames_torch(1, W, H, seed0=0, device=dev)[0]
        fr = torch.stack([torch.roll(base, (2 * i, 3 * i), dims=(0, 1)) for i in range(n)]).contiguous()
        torch.cuda.synchronize()
        ctx = pkg.Context(0, pkg.OpenCVProcessing)
        offs, _ = ctx.sift_batch_device(fr.data_ptr(), n, W, H, fr.stride(1), fr.stride(0), fetch=False)
        t0 = time.perf_counter()
        matches = ctx.match_frames(offs, pairs, ratio=0.8, cross_check=True)
        match_ms = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        verified = ctx.verify_frames(offs, pairs, matches)
        verify_ms = 1e3 * (time.perf_counter() - t0)
        d_kps = ctx.device_results()[0]

    # the C call's arguments, once
    offs64 = np.asarray(offs, np.int64)
    N = int(offs64[-1] - offs64[0])
    rec, po = ctx._match_records(matches)
    keep = np.concatenate([v[1] for v in verified]).astype(np.uint8) if len(rec) else np.zeros(1, np.uint8)
    total = int(po[-1])
    c_offs = (ctypes.c_size_t * len(offs64))(*[int(v) for v in offs64])
    c_po = (ctypes.c_size_t * len(po))(*[int(v) for v in po])
    c_pairs = (_lib.SegPair * len(pairs))(*[_lib.SegPair(x, y) for x, y in pairs])
    track_of = np.empty(max(N, 1), np.int32)
    t_offs = np.zeros(N // 2 + 2, np.uint32)
    obs = np.zeros(max(N, 1), T.OBS)
    conflict = np.zeros(N // 2 + 1, np.uint8)
    nt = ctypes.c_uint32()
    prm = _lib.TrackParams(a.min_length, 1 if a.conflicts == "drop" else 0)

    def call():
        _lib.check(pkg.lib().sift_mi_build_tracks_device(
            ctx._h, ctypes.c_void_p(d_kps), c_offs, n, c_pairs, len(pairs), rec.ctypes.data, c_po, keep.ctypes.data,
            ctypes.byref(prm), track_of.ctypes.data, ctypes.byref(nt), t_offs.ctypes.data, obs.ctypes.data,
            conflict.ctypes.data))

    with limit(120, "tracks"):
        call()  # grows the scratch
        ctx.reset_stats()
        wall, kern = [], []
        for _ in range(a.steps):
            k0 = ctx.track_counters()["kernel_ms"]
            t0 = time.perf_counter()
            call()
            wall.append(1e3 * (time.perf_counter() - t0))
            kern.append(ctx.track_counters()["kernel_ms"] - k0)
        edges = ctx.track_counters()["edges"] // a.steps
        py = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            got = ctx.track_frames(offs, pairs, matches, keep=verified, min_length=a.min_length,
                                   conflicts=a.conflicts)
            py.append(1e3 * (time.perf_counter() - t0))
    k = nt.value
    members = int(t_offs[k])

    check_ms = 0.0
    if total:
        bad = rec.copy()
        bad["query_idx"][total - 1] = -1
        chk = []
        for _ in range(a.steps + 1):
            t0 = time.perf_counter()
            rc = pkg.lib().sift_mi_build_tracks_device(
                ctx._h, ctypes.c_void_p(d_kps), c_offs, n, c_pairs, len(pairs), bad.ctypes.data, c_po,
                keep.ctypes.data, ctypes.byref(prm), track_of.ctypes.data, ctypes.byref(nt), t_offs.ctypes.data,
                obs.ctypes.data, conflict.ctypes.data)
            chk.append(1e3 * (time.perf_counter() - t0))
            if rc != -1:
                raise RuntimeError(f"the call with a bad last match returned {rc}")
        check_ms = float(np.median(chk[1:]))

    def copy_ms(nbytes, to_device):
        host = torch.empty(max(nbytes, 1), dtype=torch.uint8)  # pageable
        devb = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        ms = []
        for _ in range(a.steps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            (devb if to_device else host).copy_(host if to_device else devb)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ms[1:]))

    with limit(60, "copies"):
        up_bytes = 13 * total
        down_bytes = 4 * N + 4 * (k + 1) + k + 16 * members
        upload_ms, download_ms = copy_ms(up_bytes, True), copy_ms(down_bytes, False)

    case = dict(offsets=offs64, pairs=pairs, matches=rec[:total].astype(T.MATCH), pair_offsets=po,
                keep=keep[:total] if total else None)
    kps = shard.device_results(ctx)[0].cpu().numpy()
    t0 = time.perf_counter()
    want = T.run(case, kps=kps, min_length=a.min_length, drop_conflicts=a.conflicts == "drop")
    ref_ms = 1e3 * (time.perf_counter() - t0)
    mine = dict(track_of=track_of[:N], offsets=t_offs[:k + 1], obs=obs[:members], conflict=conflict[:k])
    exact = T.equal(mine, want) and np.array_equal(got.track_of, want["track_of"]) and \
        got.obs.tobytes() == want["obs"].tobytes()
    ea, eb = T.edges(case["offsets"], pairs, case["matches"], po, case["keep"])
    uf_ms = union_find_baseline(N, ea, eb)

    length = np.diff(t_offs[:k + 1].astype(np.int64))
    bins = [2, 3, 4, 8, 16, 32, 64, 128, 1 << 31]
    hist = {f"{lo}..{hi - 1}" if hi < (1 << 31) else f"{lo}+": int(((length >= lo) & (length < hi)).sum())
            for lo, hi in zip(bins, bins[1:])}
    call_ms, kernel_ms = float(np.median(wall)), float(np.median(kern))
    print(json.dumps({
        "what": "feature tracks over the verified matches of a device-resident batch",
        "frames": n, "frame": f"{W}x{H}", "pairs": len(pairs), "keypoints": N, "matches": total, "edges": int(edges),
        "min_length": a.min_length, "conflicts": a.conflicts, "steps": a.steps,
        "match_frames_ms": match_ms, "verify_frames_ms": verify_ms,
        "call_ms": call_ms, "all_call_ms": wall, "kernel_ms": kernel_ms,
        "upload_ms": upload_ms, "upload_bytes": up_bytes, "download_ms": download_ms, "download_bytes": down_bytes,
        "upload_share_of_call": upload_ms / call_ms, "download_share_of_call": download_ms / call_ms,
        "kernel_share_of_call": kernel_ms / call_ms,
        "index_check_ms": check_ms, "index_check_share_of_call": check_ms / call_ms,
        "rest_ms": call_ms - kernel_ms - upload_ms - download_ms - check_ms,
        "python_track_frames_ms": float(np.median(py)),
        "tracks": k, "observations": members, "length_histogram": hist,
        "longest": int(length.max()) if k else 0, "conflict_share": float(conflict[:k].mean()) if k else 0.0,
        "numpy_restatement_ms": ref_ms, "bit_exact_with_restatement": bool(exact),
        "cpp_union_find_single_thread_ms": uf_ms}))
    ctx.close()
    return 0 if exact else 1


if __name__ == "__main__":
    sys.exit(main())
