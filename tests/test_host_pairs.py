"""The host step of the frame-pair proposal (sift-features_amd/csrc/
pair_propose.h) as a stand-alone program: built with the host compiler under
AddressSanitizer and UBSan (tests/host_pairs_main.cpp), run as a subprocess on
score matrices with many equal scores, and compared with the restatement's
proposal.  No GPU, and no sanitizer runtime inside Python."""
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT

import pairs_ref as R
from test_host_tracks import _compilers

CSRC = os.path.join(ROOT, "sift-features_amd", "csrc")


def _cases():
    out = {}
    for v in ("s_min", "rank_tie_high", "keep_both"):
        inp, kw = R.fixture(v)
        out[v] = (inp["scores"], kw["min_matches"], kw.get("max_partners", 0))
    rng = np.random.default_rng(31)
    for n in (0, 1, 2, 3, 17, 64):
        for mp in (0, 1, 2, 5, 100):
            sc = rng.integers(0, 12, (n, n)).astype(np.uint32)  # few values: ties in every ranking
            out[f"random_{n}_{mp}"] = (sc, int(rng.integers(1, 10)), mp)
    out["top_of_range"] = (np.full((3, 3), 0xFFFFFFFF, np.uint32), 0xFFFFFFFF, 1)
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.fixture(scope="module", params=_compilers(), ids=os.path.basename)
def output(request, cases, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pairs")
    exe, data = str(tmp / "host_pairs"), str(tmp / "cases.txt")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param).startswith("g++") else []
    subprocess.check_call([request.param, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", *static, "-I", CSRC,
                           os.path.join(ROOT, "tests", "host_pairs_main.cpp"), "-o", exe])
    with open(data, "w") as f:
        for name, (sc, mm, mp) in cases.items():
            f.write(f"case {name} {len(sc)} {mm} {mp}\n")
            f.write(" ".join(str(int(v)) for v in np.asarray(sc).reshape(-1)) + "\n")
    run = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = {}
    for line in run.stdout.splitlines():
        _, name, *rest = line.split()
        rec[name] = [(int(a), int(b)) for a, b in zip(rest[::2], rest[1::2])]
    return rec


def test_pairs_equal_the_restatement(output, cases):
    assert set(output) == set(cases)
    for name, (sc, mm, mp) in cases.items():
        assert output[name] == R.propose(sc, mm, mp), name
    assert output["keep_both"] == [(0, 1), (0, 2), (0, 3)] and output["rank_tie_high"] == [(0, 1), (1, 3), (2, 3)]
    assert any(len(v) > 100 for v in output.values())
