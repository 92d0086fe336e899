"""The result-state rule of a context (sift-features_amd/csrc/result_state.h:
where the last result lives, which calls may read it, what a failed call
leaves) as a stand-alone program: the header api.cpp and pipeline.cpp use,
built with the host compiler under AddressSanitizer and UBSan
(tests/host_result_state_main.cpp), run as a subprocess and compared with the
restatement of the contract (tests/call_model.py) line for line.  No GPU, and
no sanitizer runtime inside Python.

  * every call sequence of 1..4 calls over the model's 21-letter alphabet
    (21 + 21^2 + 21^3 + 21^4 = 204,204 sequences: both extractions as one chunk,
    as several, refused for their arguments and failing late; precompute and
    sift_with_precomputed with the three outcomes; the four reads; both keep
    settings; set_max_octaves);
  * RANDOM_WORDS = 2,000 seeded random sequences of 12 calls: a producing call
    is 14 of 21 letters, so a word holds about 8 of them and the sample runs
    about 16,000 state changes followed by 8,000 reads at depths the
    enumeration does not reach;
  * six wrong-on-purpose variants of the header, one broken transition each:
    every one must disagree with the model on an enumerated sequence, which
    shows the enumeration sees each rule.  Variants 1-3 are what the library
    did before the header existed (fetch / device_results consulting the keep
    setting, the setting deciding where the last result is read from)."""
import os
import random
import subprocess

import pytest
from conftest import ROOT

import call_model as M
from test_host_tracks import _compilers

CSRC = os.path.join(ROOT, "sift-features_amd", "csrc")
RANDOM_WORDS, RANDOM_LEN, SEED = 2000, 12, 20241022
VARIANTS = {1: "fetch consults keep", 2: "device_results consults keep", 3: "set_keep moves where",
            4: "precompute keeps where", 5: "a late failure keeps pyramid", 6: "set_max_octaves keeps batch_readback"}
# the call sequences of the four defects the header fixed (call_model.ALPHABET)
DEFECTS = {"KaF": "fetch after a host-frame call under keep = 1",
           "KeaD": "device_results after a later host-frame call", "KekF": "fetch after a device-kept call and keep = 0", "actF": "a refused call zeroed the row count",
           "prP": "a failed precompute kept the earlier pyramid"}


@pytest.fixture(scope="module")
def words():
    rng = random.Random(SEED)
    letters = sorted(M.ALPHABET)
    sample = ["".join(rng.choice(letters) for _ in range(RANDOM_LEN)) for _ in range(RANDOM_WORDS)]
    return list(M.words(4)) + sample


@pytest.fixture(scope="module")
def expected(words):
    return [M.line(w) for w in words]


@pytest.fixture(scope="module", params=_compilers(), ids=os.path.basename)
def program(request, words, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("result_state")
    exe, data = str(tmp / "host_result_state"), str(tmp / "words.txt")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(request.param).startswith("g++") else []
    subprocess.check_call([request.param, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", *static, "-I", CSRC,
                           os.path.join(ROOT, "tests", "host_result_state_main.cpp"), "-o", exe])
    with open(data, "w") as f:
        f.write("\n".join(words) + "\n")

    def run(variant):
        r = subprocess.run([exe, str(variant), data], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()

    return run


def test_alphabet_covers_the_table():
    calls = {(c, o) for c, o, _ in M.ALPHABET.values()}
    for c in M.PRODUCING:
        assert {(c, "ok"), (c, "bad"), (c, "late")} <= calls
    assert {c for c, _ in calls} == set(M.PRODUCING) | set(M.NEEDS) | {"set_keep", "set_max_octaves"}
    chunks = {(c, a) for c, o, a in M.ALPHABET.values() if o == "ok" and c.startswith("extract")}
    assert chunks == {("extract", True), ("extract", False), ("extract_device", True), ("extract_device", False)}
    assert len(M.ALPHABET) == 21


def test_header_equals_the_model(program, words, expected):
    got = program(0)
    assert len(got) == len(words) == 21 + 21 ** 2 + 21 ** 3 + 21 ** 4 + RANDOM_WORDS
    bad = [(g, e) for g, e in zip(got, expected) if g != e]
    assert not bad, (len(bad), bad[:5])


def test_defect_sequences(program, words, expected):
    """The sequences of the four defects, by name: what the contract says of them."""
    got = dict(zip(words, program(0)))
    want = {"KaF": "KaF 0,0,0:2 host 2 011", "KeaD": "KeaD 0,0,0,S host 3 011", "KekF": "KekF 0,0,0,S device 2 010",
            "actF": "actF 0,V,S,0:1 host 1 010", "prP": "prP 0,L,S none 0 000"}
    assert set(want) == set(DEFECTS)
    for w, text in want.items():
        assert got[w] == text == M.line(w), (w, DEFECTS[w])


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_wrong_variant_is_caught(program, words, expected, variant):
    n_enum = len(words) - RANDOM_WORDS
    got = program(variant)
    caught = [w for w, g, e in zip(words[:n_enum], got, expected) if g != e]
    sample = sum(g != e for g, e in zip(got[n_enum:], expected[n_enum:]))
    print(f"variant {variant} ({VARIANTS[variant]}): {len(caught)} of {n_enum} enumerated sequences disagree, "
          f"the shortest {min(caught, key=len) if caught else None}; {sample} of {RANDOM_WORDS} random ones")
    assert caught, f"no enumerated sequence distinguishes the variant: {VARIANTS[variant]}"
