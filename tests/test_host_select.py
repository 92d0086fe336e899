"""The per-pair rule of the spread-limited selection (sift-features_amd/csrc/
select_rule.h: the suppressor test, the unfused squared distance, the host's
checks and sel_offsets) as a stand-alone program: the header select.hip
includes, built with the host compiler under AddressSanitizer and UBSan
(tests/host_select_main.cpp), run as a subprocess on the fixtures and compared
with the restatement bit for bit.  No GPU, and no sanitizer runtime inside
Python."""
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT

import select_ref as R
from test_host_tracks import _compilers

CSRC = os.path.join(ROOT, "sift-features_amd", "csrc")


def _cases():
    """name -> (kps, offsets, limit, c)"""
    out = {}
    for v in R.VARIANTS:
        (kps, offs), kw = R.fixture(v)
        out[v] = (kps, offs, kw["limit"], kw["c"])
    for kind in ("grid", "float"):
        kps, offs = R.arena([0, 1, 2, 63, 64, 65, 257, 0, 300], 17, kind)
        for limit in (1, 2, 64, 2 ** 31 - 1):
            for c in (0.9, 1.0, 0.5):
                out[f"{kind}_{limit}_{c}"] = (kps, offs, limit, c)
    kps, offs = R.bait_arena([40, 1, 0, 33, 2, 70], 5)
    out["bait"] = (kps, offs, 8, 0.9)
    out["none"] = (np.zeros((0, 5), np.float32), np.array([0], np.int64), 5, 0.9)
    return out


BAD = {  # name -> (offsets, limit, c): refused by the checks
    "limit0": ([0, 2], 0, 0.9), "c0": ([0, 2], 1, 0.0), "c_above": ([0, 2], 1, 1.5), "c_nan": ([0, 2], 1, float("nan")),
    "decreasing": ([0, 2, 1], 1, 0.9),
}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.fixture(scope="module", params=_compilers(), ids=os.path.basename)
def output(request, cases, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("select")
    exe, data = str(tmp / "host_select"), str(tmp / "cases.txt")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param).startswith("g++") else []
    subprocess.check_call([request.param, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I", CSRC,
                           os.path.join(ROOT, "tests", "host_select_main.cpp"), "-o", exe])
    with open(data, "w") as f:
        def case(name, kps, offs, limit, c):
            f.write(f"case {name} {len(offs) - 1} {limit} {int(_bits([c])[0])} {len(kps)}\n")
            f.write(" ".join(str(int(v)) for v in offs) + "\n")
            f.write(" ".join(str(int(v)) for v in _bits(kps[:, [R.X, R.Y, R.RESPONSE]]).reshape(-1)) + "\n")
        for name, (kps, offs, limit, c) in cases.items():
            case(name, kps, offs, limit, c)
        for name, (offs, limit, c) in BAD.items():
            case(name, np.ones((3, 5), np.float32), offs, limit, c)
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = {}
    for line in run.stdout.splitlines():
        tag, name, *rest = line.split()
        rec[(tag, name)] = " ".join(rest) if tag == "error" else np.array([int(v) for v in rest], np.int64)
    return rec


def test_rule_equals_the_restatement_bit_for_bit(output, cases):
    for name, (kps, offs, limit, c) in cases.items():
        sel, rows, r2 = R.run(kps, offs, limit, c)
        assert np.array_equal(output[("sel", name)], sel), name
        assert np.array_equal(output[("rows", name)], rows), name
        assert np.array_equal(output[("r2", name)], _bits(r2)), name
    assert output[("rows", "fused")].tolist() == [0, 1]  # the unfused product, whatever the compiler's default
    assert len(output[("r2", "grid_64_0.9")]) > 700


def test_checks_refuse_bad_arguments(output):
    for name in BAD:
        assert ("error", name) in output and ("rows", name) not in output, name
    assert "limit" in output[("error", "limit0")] and "decrease" in output[("error", "decreasing")]
    for name in ("c0", "c_above", "c_nan"):
        assert "(0, 1]" in output[("error", name)]
