"""The structured patterns (tests/patterns.py) on the GPU against the oracle.

Periodic and flat images put exact ties where the photographs, synth frames
and noise have none: tied DoG extrema (the non-strict comparisons of
extremum3 / k_blur_detect / k_blur_detect_pair), gradient samples with
|dx| = |dy| (k_orient's deferral to a correctly rounded f64 angle, the
orientation bin's rounding), hundreds of bit-equal responses (features_limit's
tie order), up to 8 orientations per extremum, thousands of keypoints or tens
of thousands of plateau candidates on a fresh context's first-call buffer
bounds, and empty frames between dense ones in a batch.
tests/test_patterns_cpu.py shows on the CPU that these images tell the wrong
variants of each decision from the right one, and that the older inputs do not.

Every tolerance is test_gpu_parity.assert_parity's; on top of it the response
column is bit-identical (no exp / pow in it; the limit test depends on that).
"""
import ctypes

import numpy as np
import pytest

import patterns
from test_gpu_fused import MODES
from test_gpu_parity import assert_parity
from test_patterns_cpu import COUNTS

pytestmark = pytest.mark.gpu

_oracle_memo = {}


def _oracle(oracle, name, profile, limit=None):
    """The oracle's (keypoints, descriptors, internal) of a pattern: computed
    once, shared by every test of this module, never modified."""
    key = (name, profile, limit)
    if key not in _oracle_memo:
        r = oracle.sift(patterns.make(name), features_limit=limit, profile=profile, internal=True)
        for a in r:
            a.setflags(write=False)
        _oracle_memo[key] = r
    return _oracle_memo[key]


def _processing(pkg, profile):
    return pkg.OpenCVProcessing if profile == 0 else pkg.ImageprocProcessing


@pytest.fixture(scope="module")
def contexts(pkg):
    """One context per (profile, detection form, exact): made on first use,
    closed after the module."""
    made = {}

    def get(profile, mode=None, exact=False):
        key = (profile, mode, exact)
        if key not in made:
            c = pkg.Context(0, _processing(pkg, profile))
            for k, v in (MODES[mode] if mode else {}).items():
                c.set_path_option(k, v)
            if exact:
                c.set_exact_descriptors(True)
            made[key] = c
        return made[key]

    yield get
    for c in made.values():
        c.close()


def _assert_response_bits(res, kp_o):
    assert np.array_equal(res.keypoints_array[:, 4].view(np.uint32), kp_o[:, 4].view(np.uint32)), (
        np.flatnonzero(res.keypoints_array[:, 4] != kp_o[:, 4])[:5])


def _assert_oracle(pkg, res, o):
    kp_o, desc_o, ext_o = o
    assert_parity(pkg, res, kp_o, desc_o, ext_o)
    if len(kp_o):
        _assert_response_bits(res, kp_o)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("name", patterns.names())
def test_pattern_parity(pkg, oracle, contexts, name, profile, mode):
    """Every pattern, both profiles, the four detection forms (fused pair,
    pair unrolled once, fused single column, blur and scan apart).
    Measured on MI355X (profiles/patterns_figures.md): response bit-identical
    everywhere; default-mode descriptors byte-identical on every pattern but
    rings (99.94 %), blocks4 and drift_mosaic (99.998 %) in the imageproc
    profile, max |d| 1: no pattern needs an exemption from assert_parity's
    99 % share."""
    kp_o, desc_o, ext_o = _oracle(oracle, name, profile)
    res = contexts(profile, mode).sift(patterns.make(name))  # raises unless SIFT_MI_OK
    if len(res) == len(kp_o) > 0:  # the figures, before anything is asserted
        dd = np.abs(res.descriptors.astype(np.int32) - desc_o.astype(np.int32))
        bits = np.array_equal(res.keypoints_array[:, 4].view(np.uint32), kp_o[:, 4].view(np.uint32))
        print(f"\nPATTERN {name} profile {profile} {mode}: n {len(res)} identical-byte share "
              f"{(dd == 0).mean():.5f} max|d| {dd.max()} response bit-identical {bits}")
    if name in patterns.ZERO_KEYPOINTS:
        assert len(kp_o) == 0 and len(res) == 0
    assert len(kp_o) == COUNTS[name][profile]
    _assert_oracle(pkg, res, (kp_o, desc_o, ext_o))


@pytest.mark.parametrize("name,profile", [(n, p) for n in patterns.names() for p in (0, 1) if COUNTS[n][p] > 0])
def test_pattern_exact_descriptors(pkg, oracle, contexts, name, profile):
    """set_exact_descriptors(True): descriptors byte-identical to the oracle."""
    kp_o, desc_o, ext_o = _oracle(oracle, name, profile)
    res = contexts(profile, exact=True).sift(patterns.make(name))
    _assert_oracle(pkg, res, (kp_o, desc_o, ext_o))
    assert np.array_equal(res.descriptors, desc_o), (res.descriptors != desc_o).sum()


@pytest.mark.parametrize("name", ["checker5", "squares", "diamonds", "tiled32"])
def test_pattern_limit_cuts_a_tie(pkg, ctx, oracle, name):
    """features_limit inside, at the start and at the end of the largest group
    of bit-equal responses: ties keep emission order (order.hip
    k_make_resp_keys / k_select), through sift() and a batch of three copies."""
    img = patterns.make(name)
    kp_all = _oracle(oracle, name, 0)[0]
    groups, _ = patterns.response_groups(kp_all[:, 4])
    a, b = max(groups, key=lambda g: g[1] - g[0])
    assert b - a >= 2  # a precondition on the oracle's result, not a measurement
    for limit in (a, (a + b) // 2, b):
        o = _oracle(oracle, name, 0, limit)
        assert len(o[0]) == limit
        res = ctx.sift(img, features_limit=limit)
        _assert_oracle(pkg, res, o)
        batch = ctx.sift_batch(np.stack([img] * 3), features_limit=limit)
        assert len(batch) == 3
        for f, r in enumerate(batch):
            _assert_oracle(pkg, r, o)
            assert r == res
            assert np.array_equal(pkg.key_fields(r.keys)["frame"], np.full(limit, f))


MIXED = ["checker5", "white_96x128", "diamonds", "flat77_96x128", "drift_mosaic", "blocks4", "step_96x128"]
MIXED_EMPTY = (1, 3, 6)


def _batch_with_offsets(pkg, c, frames, limit):
    """Context.sift_batch, keeping the per-frame offsets the C ABI returns."""
    f = np.ascontiguousarray(frames, dtype=np.uint8)
    n, h, w = f.shape
    ptrs = (ctypes.c_void_p * n)(*[f[i].ctypes.data for i in range(n)])
    offs = (ctypes.c_size_t * (n + 1))()
    rc = pkg.lib().sift_mi_extract_batch(c._h, ptrs, n, w, h, w, -1 if limit is None else limit, offs)
    assert rc == 0, (rc, pkg.lib().sift_mi_last_error())
    offs = [int(v) for v in offs]
    kps, desc, keys = c._fetch(offs[n])
    return offs, [pkg.SiftResult(kps[offs[i]:offs[i + 1]], desc[offs[i]:offs[i + 1]], keys[offs[i]:offs[i + 1]])
                  for i in range(n)]


@pytest.mark.parametrize("limit", [None, 40])
@pytest.mark.parametrize("chunking", ["one_chunk", "chunk2_lanes1", "chunk2_lanes2"])
@pytest.mark.parametrize("profile", [0, 1])
def test_pattern_batch_mixed(pkg, oracle, contexts, profile, chunking, limit):
    """Dense, empty, dense, empty, dense (the drift fixture), dense, empty:
    zero-keypoint frames between dense ones and at the end of a batch
    (k_frame_starts, k_limit_plan, equal consecutive offsets); with chunk 2
    the seven frames leave a last chunk of one frame, the empty one."""
    frames = np.stack([patterns.make(n) for n in MIXED])
    c = pkg.Context(0, _processing(pkg, profile))
    try:
        if chunking == "one_chunk":
            c.set_chunk(len(MIXED))
        else:
            c.set_chunk(2)
            c.set_pipeline_lanes(1 if chunking == "chunk2_lanes1" else 2)
        offs, got = _batch_with_offsets(pkg, c, frames, limit)
    finally:
        c.close()
    single = contexts(profile)
    want = []
    for i, name in enumerate(MIXED):
        o = _oracle(oracle, name, profile, limit)
        _assert_oracle(pkg, got[i], o)
        assert got[i] == single.sift(frames[i], features_limit=limit), name
        assert np.array_equal(pkg.key_fields(got[i].keys)["frame"], np.full(len(got[i]), i))
        want.append(len(o[0]))
    assert offs[0] == 0 and np.all(np.diff(offs) >= 0)
    assert list(np.diff(offs)) == want
    for i in MIXED_EMPTY:  # the empty frames, the last one included
        assert offs[i] == offs[i + 1]
    assert offs[len(MIXED) - 1] == offs[len(MIXED)] == sum(want)
    assert all(want[i] > 0 for i in range(len(MIXED)) if i not in MIXED_EMPTY)


@pytest.mark.parametrize("shrink", [1, 1000])
@pytest.mark.parametrize("entry", ["sift", "batch3"])
@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("name", ["checker5", "white"])
def test_pattern_first_call_bounds(pkg, oracle, name, profile, entry, shrink):
    """A fresh context has no high-water marks: its buffers are sized by
    chunk_bounds' first-call estimates (pipeline.cpp: 1.3 * sum(px) / 256
    candidates, / 512 extrema, / 384 keypoints, each + 1024; bound_shrink =
    1000 divides them and drops the slack).  checker5 (OpenCV profile) has
    3188 keypoints against a bound of 1245; `white` has tens of thousands of
    plateau candidates (test_patterns_cpu.test_plateau_candidates) against
    1446, and ends with no keypoint.  finalize_chunk re-runs a chunk whose
    candidate count h[0] exceeds S.bc (the scan counts every candidate and
    stores only those below the bound), so `white` re-runs under the default
    options too.  Each re-run learns one more stage's true count (candidates,
    then extrema, then keypoints), so the four attempts always suffice; the
    call never returns SIFT_MI_ENOMEM."""
    img = patterns.make(name)
    o = _oracle(oracle, name, profile)
    c = pkg.Context(0, _processing(pkg, profile))
    try:
        if shrink > 1:
            c.set_path_option("bound_shrink", shrink)
        if entry == "sift":
            run = lambda: [c.sift(img)]
        else:
            c.set_chunk(2)
            c.set_pipeline_lanes(2)
            run = lambda: c.sift_batch(np.stack([img] * 3))
        first = run()  # SIFT_MI_ENOMEM would raise SiftMiError here
        reruns = c.stats()["stage_reruns"]
        second = run()
        reruns2 = c.stats()["stage_reruns"] - reruns
    finally:
        c.close()
    print(f"\nFIRSTCALL {name} profile {profile} {entry} bound_shrink {shrink}: stage_reruns {reruns} "
          f"(second call {reruns2})")
    for r in first:
        _assert_oracle(pkg, r, o)
    assert len(first) == len(second) and all(a == b for a, b in zip(first, second))
    if name == "white":
        assert all(len(r) == 0 for r in first)
    if shrink > 1 or name == "white" or profile == 0:
        assert reruns >= 1, reruns
    assert reruns2 == 0, reruns2  # the bounds are learned


@pytest.mark.parametrize("n_bands", [2, 3])
@pytest.mark.parametrize("name", ["checker5", "squares", "border_mosaic"])
def test_pattern_row_bands(pkg, ctx, name, n_bands):
    """A tied extremum on a band's boundary row is emitted by exactly one
    band: the union of the bands, ordered by key, is the whole frame.
    border_mosaic: k_refine's vlo / vhi rows and the band-seam re-run meet
    the image-border rules of its moves."""
    from test_gpu_bands import _assert_whole, _bands
    img = patterns.make(name)
    whole = ctx.sift(img)
    assert len(whole) == COUNTS[name][0]
    parts = _bands(ctx, img, n_bands)
    assert sum(len(p[2]) for p in parts) == len(whole)
    _assert_whole(parts, whole)
    assert ctx.sift(img) == whole
