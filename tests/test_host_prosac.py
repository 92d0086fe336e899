"""The host side of the progressive sampling (sift-features_amd/csrc/
prosac_growth.h: the growth table and the quality check) as a stand-alone
program: built with the host compilers under AddressSanitizer and UBSan
(tests/host_prosac_main.cpp), run as a subprocess, and compared with
prosac_ref.py integer for integer.  No GPU, and no sanitizer runtime inside
Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT

import prosac_ref as P

CSRC = os.path.join(ROOT, "sift-features_amd", "csrc")
N_MAX = 2049
KS = (4, 8)
TS = (1, 255, 1024, 65536)


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
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("prosac") / "host_prosac")
    # (the sanitizer runtimes linked into the program itself: clang's default)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param).startswith("g++") else []
    subprocess.check_call([request.param, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I", CSRC,
                           os.path.join(ROOT, "tests", "host_prosac_main.cpp"), "-o", path])
    return path


def test_a_host_compiler_is_present():
    assert _compilers(), "neither g++ nor the ROCm clang++ found"


def growth_all(k, T, n_max):
    """T'[N, n] for every N = 0..n_max at once: prosac_ref.growth's operations,
    one numpy f64 operation each, elementwise over N (rows N < k stay 0)."""
    N = np.arange(n_max + 1, dtype=np.float64)
    live = np.arange(n_max + 1) >= k
    t = np.full(n_max + 1, float(T))
    with np.errstate(all="ignore"):
        for i in range(k):
            t = t * float(k - i)
            t = t / (N - float(i))
        tp = np.zeros((n_max + 1, n_max + 1), np.int64)
        tp[live, k] = 1
        for n in range(k, n_max):
            t1 = t * float(n + 1)
            t1 = t1 / float(n + 1 - k)
            step = np.ceil(t1 - t)
            rows = np.arange(n_max + 1) >= n + 1  # N > n: the pairs that have a T'_{n+1}
            tp[rows, n + 1] = tp[rows, n] + step[rows].astype(np.int64)
            t = t1
    return tp


def test_growth_all_is_the_restatement():
    for k in KS:
        for T in TS:
            tp = growth_all(k, T, 300)
            for N in list(range(0, k + 12)) + [63, 64, 65, 255, 299, 300]:
                assert tp[N, :N + 1].tolist() == P.growth(N, k, T), (k, T, N)
    tp = growth_all(8, 1024, N_MAX)
    for N in (1023, 1025, 2048, 2049):
        assert tp[N, :N + 1].tolist() == P.growth(N, 8, 1024), N


def test_tables_equal_the_restatement(exe, tmp_path):
    """Every N from k to 2049 at 1, 255, 1024 and 65536 iterations, both sample sizes."""
    out = str(tmp_path / "tables.bin")
    run = subprocess.run([exe, "tables", out, str(N_MAX)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    got = np.fromfile(out, np.uint32)
    os.remove(out)
    at = 0
    for k in KS:
        for T in TS:
            tp = growth_all(k, T, N_MAX)
            for N in range(k, N_MAX + 1):
                tab = got[at:at + N]
                at += N
                assert not tab[:k - 1].any(), (k, T, N)
                assert np.array_equal(tab[k - 1:], tp[N, k:N + 1]), (k, T, N)
            assert tp.max() <= T + N_MAX
    assert at == len(got)


def test_quality_check(exe):
    run = subprocess.run([exe, "quality"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [ln.split()[1:] for ln in run.stdout.splitlines()]
    assert lines.pop() == ["empty", "0"]
    assert len(lines) == 11
    for bits, plain, strided, before in lines:
        v = np.array([int(bits, 16)], np.uint32).view(np.float32)
        want = 1 if not np.isfinite(v[0]) else 2 if np.signbit(v[0]) else 0
        try:
            P.check_quality(v)
            assert want == 0, bits
        except ValueError:
            assert want != 0, bits
        assert (int(plain), int(strided), int(before)) == (want, want, 0), bits  # the offender is entry 3
    assert sorted({ln[1] for ln in lines}) == ["0", "1", "2"]


def test_a_pair_near_the_row_limit(exe):
    """N = 2^31 - 1, the most a call accepts, stepped without a table: the
    first entries and the last.  Every step is 1 there
    (test_prosac_ref_cpu.py::test_growth_steps_of_one_for_a_huge_pair), so
    T'_N = N - k + 1, which still fits the table's u32.  The 2^31 steps are
    one chain of dependent multiplies and divides, by far the longest case of
    this file, so it is one case (k = 8) under the first compiler only; the
    other compiler's program runs a pair of 2^20 matches through the same
    steps."""
    first_compiler = os.path.basename(exe) == os.path.basename(_compilers()[0])
    N = 2**31 - 1 if first_compiler else 2**20
    for k in (8,):
        run = subprocess.run([exe, "huge", str(N), str(k), "65536"], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]
        got = [int(x) for x in run.stdout.split()[1:]]
        first = P.growth(N, k, 65536, stop=k + 2)[k:]
        assert got == [N, k, *first, N - k + 1]
        assert first == [1, 2, 3]
