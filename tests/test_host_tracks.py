"""The track builder's lock-free union-find (sift-features_amd/csrc/
track_common.h) as a stand-alone program: the header instantiated with
std::atomic, run from 8 threads released together over the fixtures' edge lists, built with the
host compiler under AddressSanitizer and UBSan (tests/host_tracks_main.cpp),
run as a subprocess, and compared with the restatement's labels.  The program
aborts if a walk or a union exceeds its bound.  No GPU, and no sanitizer
runtime inside Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT

import tracks_ref as T

CSRC = os.path.join(ROOT, "sift-features_amd", "csrc")


def _graphs():
    g = {
        "chain": T.chain(40, per_seg=3),
        "chain_reversed": T.chain(128, reverse=True),
        "hub": T.hub(4096),
        "star": T.star(4096),
        "random": T.random_graph(T.SEG_LENS, 20, 0.5, 1, base=5, keep_share=0.8),
        "dense": T.random_graph([50, 50], 30, 1.0, 2),
        "panning": T.panning(16, 80, 4),
        "empty": T.case([3, 0, 2], [], []),
        "none": T.case([], [], []),
    }
    return {k: (int(c["offsets"][-1] - c["offsets"][0]),
                *T.edges(c["offsets"], c["pairs"], c["matches"], c["pair_offsets"], c["keep"])) for k, c in g.items()}


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


@pytest.fixture(scope="module")
def graphs():
    return _graphs()


@pytest.fixture(scope="module", params=_compilers(), ids=os.path.basename)
def output(request, graphs, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tracks")
    exe, data = str(tmp / "host_tracks"), str(tmp / "graphs.txt")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param).startswith("g++") else []
    subprocess.check_call([request.param, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", *static, "-I", CSRC,
                           os.path.join(ROOT, "tests", "host_tracks_main.cpp"), "-o", exe, "-lpthread"])
    with open(data, "w") as f:
        for name, (n, a, b) in graphs.items():
            f.write(f"graph {name} {n} {len(a)}\n")
            f.writelines(f"{x} {y}\n" for x, y in zip(a.tolist(), b.tolist()))
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = {}
    for line in run.stdout.splitlines():
        tag, name, *rest = line.split()
        rec[(tag, name)] = [int(v) for v in rest]
    return rec


def test_a_host_compiler_is_present():
    assert _compilers(), "neither g++ nor the ROCm clang++ found"


def test_labels_equal_the_restatement(output, graphs):
    for name, (n, a, b) in graphs.items():
        assert np.array_equal(np.array(output[("labels", name)], np.int64), T.labels(n, a, b)), name


def test_both_bounds_were_live(output, graphs):
    """The program counted steps and retries (it aborts past either bound): a
    path walks, and on the hub, whose 4096 edges all link the same root from
    8 threads released together, links lost their race and retried."""
    steps, _ = output[("steps", "chain_reversed")]
    assert steps > 0
    steps, retries = output[("steps", "hub")]
    assert steps > 0 and retries > 0
    assert output[("steps", "none")] == [0, 0]
