"""The library's host arithmetic (sift-features_amd/csrc/geometry.cpp) as a
stand-alone program: built with the host compiler under AddressSanitizer and
UBSan (tests/host_geometry_main.cpp), run as a subprocess, and compared with
the CPU oracle bit for bit.  No GPU, and no sanitizer runtime inside Python.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT

CSRC = os.path.join(ROOT, "sift-features_amd", "csrc")
FRAMES = [(1, 1), (2, 3), (16, 16), (97, 161), (640, 480), (1920, 1080), (8192, 8192), (16384, 1)]
IMAGES = 6
MARGIN = 24 + 1 + 41  # kBandDrift + 1 + kBandPatch


def _compilers():
    out = []
    gxx = shutil.which("g++")
    if gxx:
        out.append(gxx)
    for cand in (shutil.which("amdclang++"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cand and os.path.exists(cand):
            out.append(cand)
            break
    return out


@pytest.fixture(scope="module", params=_compilers(), ids=os.path.basename)
def records(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("geometry") / "host_geometry")
    # (the sanitizer runtimes linked into the program itself: clang's default)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param).startswith("g++") else []
    subprocess.check_call([request.param, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I", CSRC,
                           os.path.join(CSRC, "geometry.cpp"), os.path.join(ROOT, "tests", "host_geometry_main.cpp"),
                           "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = {}
    for line in run.stdout.splitlines():
        tag, *rest = line.split()
        rec.setdefault(tag, []).append(rest)
    return rec


def test_a_host_compiler_is_present():
    assert _compilers(), "neither g++ nor the ROCm clang++ found"


def f32_bits(hexes):
    return np.array([float.fromhex(h) for h in hexes], np.float64).astype(np.float32).view(np.uint32)


def test_octave_count_and_sigmas(records, oracle):
    got = {(int(w), int(h)): int(n) for w, h, n in records["n_octaves"]}
    assert sorted(got) == sorted(FRAMES)
    for (w, h), n in got.items():
        assert n == oracle.n_octaves(w, h), (w, h)
    sig = [float.fromhex(x) for x in records["octave_sigmas"][0]]
    assert [s.hex() for s in sig] == [float(s).hex() for s in oracle.octave_sigmas()]
    assert float.fromhex(records["seed_sigma"][0][0]).hex() == float(oracle.seed_sigma()).hex()


def test_blur_taps_both_profiles(records, oracle):
    sigmas = [oracle.seed_sigma()] + [float(s) for s in oracle.octave_sigmas()[1:]]
    L = oracle.lib()
    L.oracle_ip_kernel.argtypes = [ctypes.c_float, ctypes.c_void_p]
    L.oracle_ip_kernel.restype = ctypes.c_int
    assert len(records["cv_taps"]) == len(records["ip_taps"]) == IMAGES
    for sigma, cv, ip in zip(sigmas, records["cv_taps"], records["ip_taps"]):
        assert float.fromhex(cv[0]).hex() == sigma.hex()
        full = oracle.cv_kernel(sigma)
        r = int(cv[1])
        assert len(full) == 2 * r + 1 and len(cv) == 2 + r + 1
        assert np.array_equal(f32_bits(cv[2:]), np.ascontiguousarray(full[r:]).view(np.uint32))
        assert np.array_equal(f32_bits(cv[2:]), np.ascontiguousarray(full[r::-1]).view(np.uint32))
        s32 = np.float32(sigma)
        assert np.float32(float.fromhex(ip[0])) == s32
        buf = np.zeros(128, np.float32)
        n = L.oracle_ip_kernel(ctypes.c_float(float(s32)), buf.ctypes.data)
        r = int(ip[1])
        assert n == 2 * r + 1 and len(ip) == 2 + r + 1
        assert np.array_equal(f32_bits(ip[2:]), buf[r:n].view(np.uint32))


def test_ip_axis_upsample_and_nearest_half(records, oracle):
    L = oracle.lib()
    L.oracle_ip_axis.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p,
                                 ctypes.c_void_p]
    L.oracle_ip_axis.restype = ctypes.c_int
    seen = set()
    for src, dst, support, out, left, n, *w in records["ip_axis"]:
        src, dst, out, left, n = int(src), int(dst), int(out), int(left), int(n)
        support = float.fromhex(support)
        seen.add((src, dst, support))
        o_left = ctypes.c_int(0)
        o_w = np.zeros(64, np.float32)
        o_n = L.oracle_ip_axis(src, dst, out, ctypes.c_float(support), ctypes.addressof(o_left), o_w.ctypes.data)
        assert (n, left) == (o_n, o_left.value), (src, dst, out)
        assert np.array_equal(f32_bits(w), o_w[:n].view(np.uint32)), (src, dst, out)
    # 2x Triangle and nearest 1/2, each at an odd and an even source size
    assert seen == {(97, 194, 1.0), (16, 32, 1.0), (97, 48, 0.0), (16, 8, 0.0)}


def test_octave_geometry(records, oracle):
    octs = {}
    for w, h, o, *v in records["octave"]:
        octs.setdefault((int(w), int(h)), []).append([int(x) for x in v])
    for w, h, ok, arena in records["geometry"]:
        w, h = int(w), int(h)
        assert ok == "1"
        rows = octs[(w, h)]
        assert len(rows) == oracle.n_octaves(w, h)
        end = 0
        for o, (ow, oh, pitch, P, px, goff, doff, near_cv, near_ip) in enumerate(rows):
            assert (ow, oh) == ((2 * w) >> o, (2 * h) >> o) and ow >= 1 and oh >= 1
            assert pitch % 64 == 0 and 0 <= pitch - ow < 64  # 256-byte rows
            assert P == pitch * oh and px == ow * oh
            assert goff == end and goff % 64 == 0  # 256-byte aligned octave arenas
            assert doff == goff + 6 * P  # the chunk's (one frame's) G_0..G_5, then one frame of D_0..D_4
            end = (doff + 5 * P + 63) // 64 * 64
            assert near_cv == 0 and near_ip == 0  # nearest 1/2 picks pixel 2x / 2x + 1
        assert int(arena) == end


def test_band_rows_keep_their_promises(records):
    radii = [0] + [int(r) for r in records["band_radii"][0]]
    assert radii[1:] == [5, 6, 8, 10, 13]  # OpenCV profile, sigmas 1.23 .. 3.09
    bands = {}
    for w, h, band_n, band_r, o, H, blo, bhi, *rows in records["band"]:
        key = (int(w), int(h), int(band_n), int(o))
        rows = [int(x) for x in rows]
        bands.setdefault(key, []).append((int(band_r), int(H), int(blo), int(bhi), rows[0::2], rows[1::2]))
    assert {k[:3] for k in bands} == {(w, h, n) for (w, h) in [(97, 161), (1920, 1080)] for n in (1, 2, 3, 8)}
    for (w, h, band_n, o), per_band in bands.items():
        assert [b[0] for b in per_band] == list(range(band_n))
        H = per_band[0][1]
        assert H == (2 * h) >> o
        # the detection rows of the bands of one octave partition [0, H)
        assert per_band[0][2] == 0 and per_band[-1][3] == H
        for a, b in zip(per_band, per_band[1:]):
            assert a[3] == b[2]
        for band_r, _, blo, bhi, lo, hi in per_band:
            assert blo <= bhi
            for s in range(IMAGES):
                # clipped to [0, H), and the margin around the detection rows
                assert 0 <= lo[s] <= hi[s] <= H
                assert lo[s] <= max(0, blo - 1 - MARGIN) and hi[s] >= min(H, bhi + 1 + MARGIN)
            for s in range(1, IMAGES):
                # blur s reads radii[s] rows of G_{s-1} around each of its rows:
                # lo[s-1] <= lo[s] - r_s and hi[s-1] >= hi[s] + r_s before the
                # clip, so after it the same against the clipped bound
                assert lo[s - 1] <= max(0, lo[s] - radii[s])
                assert hi[s - 1] >= min(H, hi[s] + radii[s])
            nxt = bands.get((w, h, band_n, o + 1))
            if nxt:  # the next octave's G_0 row y is this octave's G_3 row 2y (or 2y + 1)
                _, _, _, _, nlo, nhi = nxt[band_r]
                if nhi[0] > nlo[0]:
                    assert lo[3] <= 2 * nlo[0] and hi[3] >= min(H, 2 * nhi[0] + 1)


def test_auto_chunk_documented_cases(records):
    got = {(int(w), int(h), int(n), int(mode)): int(v) for w, h, n, mode, v in records["auto_chunk"]}
    assert got == {(1920, 1080, 128, 1): 128, (1920, 1080, 128, 0): 64,
                   (640, 480, 256, 1): 256, (640, 480, 256, 0): 128}
