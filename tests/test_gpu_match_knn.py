"""2-nearest-neighbour matching, the ratio test and segment-pair matching of
device-resident descriptors (sift_mi_match_neighbors, sift_mi_match_ratio,
sift_mi_match_pairs_device) against the CPU oracle's matcher and its numpy
restatement (match_ref.py).  Everything is bit-exact: indices equal, f32
distances equal as bit patterns."""
import ctypes
import functools

import numpy as np
import pytest
from conftest import load_golden

import match_ref

gpu = pytest.mark.gpu

SHAPES = [(1, 1), (5, 1), (1, 2), (37, 300), (128, 128), (129, 257), (300, 129)]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and \
        np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


@functools.lru_cache(maxsize=None)
def _planted(nq, nt):
    q, t = match_ref.planted(nq, nt, nq * 7 + nt)
    q.setflags(write=False)
    t.setflags(write=False)
    return q, t


@functools.lru_cache(maxsize=None)
def _ref(nq, nt, ratio, cross):
    return match_ref.match(*_planted(nq, nt), ratio, cross)


# ---- neighbours and ratio -----------------------------------------------------
@gpu
@pytest.mark.parametrize("nq,nt", SHAPES)
def test_neighbors_planted(ctx, nq, nt):
    q, t = _planted(nq, nt)
    idx, dist = ctx.match_neighbors(q, t)
    ridx, rdist = match_ref.neighbors(q, t)
    assert idx.dtype == np.int32 and dist.dtype == np.float32 and idx.shape == (nq, 2)
    assert np.array_equal(idx, ridx)
    assert np.array_equal(dist.view(np.uint32), rdist.view(np.uint32))


@gpu
@pytest.mark.parametrize("cross", [True, False])
@pytest.mark.parametrize("ratio", [0.8, 0.95, 1.0])
@pytest.mark.parametrize("nq,nt", SHAPES)
def test_ratio_planted(ctx, nq, nt, ratio, cross):
    """At 0.8 the reference alone keeps the planted third (at least a quarter
    of min(nq, nt)) and rejects at least a quarter of the queries; for
    (300, 129) the planted third of the 129 train rows is 43 of 300 queries,
    so the kept share is counted against min(nq, nt).  At 0.95 some unplanted
    queries pass too (test_match_ref_cpu.py)."""
    q, t = _planted(nq, nt)
    want = _ref(nq, nt, ratio, cross)
    if min(nq, nt) >= 37 and ratio == 0.8 and not cross:
        kept = len(want[0])
        assert 4 * kept >= min(nq, nt) and 4 * (nq - kept) >= nq, (kept, nq)
    if nt < 2:
        assert len(want[0]) == 0  # no second neighbour: rejected
    got = ctx.match_descriptors(q, t, cross_check=cross, ratio=ratio)
    assert _same(got, want), (len(got[0]), len(want[0]))


@gpu
def test_triples(ctx):
    q, t = match_ref.triples()
    idx, dist = ctx.match_neighbors(q, t)
    assert np.array_equal(idx[:, 0], np.arange(50)[::-1])
    assert np.array_equal(idx[:, 1], idx[:, 0] + 50)  # the second copy, not the third
    assert np.all(dist == 0)
    for cross in (True, False):
        assert len(ctx.match_descriptors(q, t, cross_check=cross, ratio=1.0)[0]) == 0  # strict <
        assert _same(ctx.match_descriptors(q, t, cross_check=cross, ratio=0.8),
                     match_ref.match(q, t, 0.8, cross))


@gpu
def test_self_match(ctx):
    q, _ = _planted(300, 129)
    idx, dist = ctx.match_neighbors(q, q)
    assert np.array_equal(idx[:, 0], np.arange(len(q))) and np.all(dist[:, 0] == 0)
    ridx, rdist = match_ref.neighbors(q, q)
    assert np.array_equal(idx, ridx) and np.array_equal(dist.view(np.uint32), rdist.view(np.uint32))


@gpu
@pytest.mark.parametrize("cross", [True, False])
def test_ratio_zero_equals_match_descriptors(ctx, oracle, cross):
    for nq, nt in SHAPES:
        q, t = _planted(nq, nt)
        got = ctx.match_descriptors(q, t, cross_check=cross, ratio=0.0)
        assert _same(got, ctx.match_descriptors(q, t, cross_check=cross))
        assert _same(got, oracle.match(q, t, cross_check=cross))


@gpu
def test_empty_sets(ctx):
    e = np.zeros((0, 128), np.uint8)
    x = np.ones((5, 128), np.uint8)
    for q, t in [(e, x), (x, e), (e, e)]:
        assert len(ctx.match_descriptors(q, t, ratio=0.8)[0]) == 0
        assert len(ctx.match_descriptors(q, t, cross_check=False, ratio=0.0)[0]) == 0
        idx, dist = ctx.match_neighbors(q, t)
        assert idx.shape == (len(q), 2) and np.all(idx == -1) and np.all(np.isinf(dist))


# ---- segments -------------------------------------------------------------------
SEG_LENS, PAIRS = match_ref.SEG_LENS, match_ref.PAIRS


@pytest.fixture(scope="module")
def arena_dev():
    import torch
    rows, offs = match_ref.segment_arena()
    t = torch.from_numpy(rows.copy()).cuda()
    torch.cuda.synchronize()
    return t, rows, offs


def _seg(rows, offs, s):
    return rows[offs[s]:offs[s + 1]]


@gpu
@pytest.mark.parametrize("cross", [True, False])
@pytest.mark.parametrize("ratio", [None, 0.8, 1.0])
def test_segment_pairs(ctx, oracle, arena_dev, ratio, cross):
    t, rows, offs = arena_dev
    got = ctx.match_pairs_device(t.data_ptr(), offs, PAIRS, ratio=ratio, cross_check=cross)
    assert len(got) == len(PAIRS)
    for (a, b), g in zip(PAIRS, got):
        q, tr = _seg(rows, offs, a), _seg(rows, offs, b)
        want = oracle.match(q, tr, cross_check=cross) if ratio is None else match_ref.match(q, tr, ratio, cross)
        assert _same(g, want), (a, b, len(g[0]), len(want[0]))
        if len(q) == 0 or len(tr) == 0:
            assert len(g[0]) == 0
        else:
            assert g[0].max(initial=0) < len(q) and g[1].max(initial=0) < len(tr)  # segment-relative
    assert _same(got[PAIRS.index((5, 2))], got[-1])  # the pair listed twice
    if ratio is None:
        assert len(got[PAIRS.index((3, 3))][0]) == SEG_LENS[3]  # self pair: every row matches itself


def _raw(pkg, ctx, d_ptr, offs, pairs, ratio, cross, cap):
    from sift_features_amd import _lib
    L = pkg.lib()
    c_offs = None if offs is None else (ctypes.c_size_t * len(offs))(*[int(v) for v in offs])
    c_pairs = None if pairs is None else (_lib.SegPair * max(1, len(pairs)))(*[_lib.SegPair(a, b) for a, b in pairs])
    n_pairs = 0 if pairs is None else len(pairs)
    out = (_lib.Match * max(cap, 1))()
    po = (ctypes.c_size_t * (n_pairs + 1))(*([12345] * (n_pairs + 1)))
    rc = L.sift_mi_match_pairs_device(ctx._h, ctypes.c_void_p(d_ptr), c_offs, 0 if offs is None else len(offs) - 1,
                                      c_pairs, n_pairs, ratio, cross, out, cap, po)
    return rc, out, list(po)


@gpu
def test_pair_offsets_and_cap(pkg, ctx, oracle, arena_dev):
    t, rows, offs = arena_dev
    want = [oracle.match(_seg(rows, offs, a), _seg(rows, offs, b), cross_check=True) for a, b in PAIRS]
    counts = [len(w[0]) for w in want]
    total = sum(counts)
    assert total > 0
    rc, out, po = _raw(pkg, ctx, t.data_ptr(), offs, PAIRS, 0.0, 1, total)
    assert rc == 0 and po == [0] + list(np.cumsum(counts))
    a = np.ctypeslib.as_array(out)[:total]
    assert np.array_equal(a["query_idx"], np.concatenate([w[0] for w in want]))
    assert np.array_equal(a["train_idx"], np.concatenate([w[1] for w in want]))
    # cap too small: EINVAL, the needed count in pair_offsets[n_pairs]
    rc, _, po = _raw(pkg, ctx, t.data_ptr(), offs, PAIRS, 0.0, 1, total - 1)
    assert rc == -1 and po[-1] == total
    assert b"cap" in pkg.lib().sift_mi_last_error()
    rc, _, po = _raw(pkg, ctx, t.data_ptr(), offs, PAIRS, 0.0, 1, 0)
    assert rc == -1 and po[-1] == total
    # no pairs: an empty result
    rc, _, po = _raw(pkg, ctx, t.data_ptr(), offs, [], 0.0, 1, 0)
    assert rc == 0 and po == [0]


@gpu
def test_pairs_einval(pkg, ctx, arena_dev):
    t, rows, offs = arena_dev
    L = pkg.lib()
    d, n_seg, ok_pairs, cap = t.data_ptr(), len(offs) - 1, [(1, 2)], 1000
    assert _raw(pkg, ctx, d, offs, ok_pairs, 0.8, 1, cap)[0] == 0
    # null arguments
    assert _raw(pkg, ctx, None, offs, ok_pairs, 0.8, 1, cap)[0] == -1
    assert _raw(pkg, ctx, d, None, ok_pairs, 0.8, 1, cap)[0] == -1
    assert _raw(pkg, ctx, d, offs, None, 0.8, 1, cap)[0] == -1
    from sift_features_amd import _lib
    c_offs = (ctypes.c_size_t * len(offs))(*[int(v) for v in offs])
    c_pairs = (_lib.SegPair * 1)(_lib.SegPair(1, 2))
    out = (_lib.Match * cap)()
    assert L.sift_mi_match_pairs_device(ctx._h, ctypes.c_void_p(d), c_offs, n_seg, c_pairs, 1, 0.8, 1, out, cap,
                                        None) == -1
    # matches to write but no `out`
    po = (ctypes.c_size_t * 2)()
    assert L.sift_mi_match_pairs_device(ctx._h, ctypes.c_void_p(d), c_offs, n_seg, c_pairs, 1, 0.0, 0, None, cap,
                                        po) == -1 and po[1] == 1
    # ratio: NaN, negative, above 1
    for bad in (float("nan"), -0.5, 1.0001, float("inf")):
        assert _raw(pkg, ctx, d, offs, ok_pairs, bad, 1, cap)[0] == -1, bad
        q = np.ones((3, 128), np.uint8)
        with pytest.raises(pkg.SiftMiError):
            ctx.match_descriptors(q, q, ratio=bad)
    # a pair index >= n_segs
    assert _raw(pkg, ctx, d, offs, [(1, n_seg)], 0.8, 1, cap)[0] == -1
    assert _raw(pkg, ctx, d, offs, [(n_seg, 1)], 0.8, 1, cap)[0] == -1
    # decreasing offsets
    assert _raw(pkg, ctx, d, [0, 10, 5, 20], [(0, 1)], 0.8, 1, cap)[0] == -1
    # a segment, or the sum of the segments, above 2^31 - 1 rows (rejected before any device work)
    assert _raw(pkg, ctx, d, [0, 1 << 31], [(0, 0)], 0.8, 1, cap)[0] == -1
    assert _raw(pkg, ctx, d, [0, (1 << 31) - 1, (1 << 31) + 5], [(1, 1)], 0.8, 1, cap)[0] == -1
    # still usable afterwards
    assert _raw(pkg, ctx, d, offs, ok_pairs, 0.8, 1, cap)[0] == 0


# ---- end to end -------------------------------------------------------------------
@gpu
def test_match_frames_end_to_end(pkg, ctx, oracle):
    import torch
    img = load_golden("bird_small")["image"]
    assert img.shape == (213, 320)
    frames = np.stack([img, np.roll(img, 7, axis=1), np.roll(img, (5, -9), axis=(0, 1))])
    host = ctx.sift_batch(frames)
    t = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    c2 = pkg.Context(0, pkg.OpenCVProcessing)
    try:
        offs, res = c2.sift_batch_device(t.data_ptr(), 3, 320, 213, t.stride(1), t.stride(0), fetch=False)
        assert res is None and [int(offs[i + 1] - offs[i]) for i in range(3)] == [len(r) for r in host]
        before = c2.device_results()
        pairs = [(0, 1), (1, 2), (0, 2)]
        first = c2.match_frames(offs, pairs)
        for (a, b), g in zip(pairs, first):
            want = oracle.match(host[a].descriptors, host[b].descriptors, cross_check=True)
            assert _same(g, want), (a, b)
            assert len(g[0]) > 20
        again = c2.match_frames(offs, pairs)
        assert all(_same(x, y) for x, y in zip(first, again))
        assert c2.device_results() == before
        desc = np.empty((before[2], 128), np.uint8)
        hip = ctypes.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(ctypes.c_void_p(desc.ctypes.data), ctypes.c_void_p(before[1]), desc.nbytes, 2) == 0
        assert np.array_equal(desc, np.concatenate([r.descriptors for r in host]))
        ratio = c2.match_frames(offs, pairs, ratio=0.8)
        for (a, b), g in zip(pairs, ratio):
            assert _same(g, match_ref.match(host[a].descriptors, host[b].descriptors, 0.8, True)), (a, b)
    finally:
        c2.close()


@gpu
def test_sift_match_cli(pkg, ctx, oracle):
    """sift_match.py, the examples/sift-match.rs counterpart: both keypoint
    counts and the cross-checked matches of the second image's descriptors
    against the first's (the snapshot counts with --processing opencv:
    src/snapshots, 225 / 1270)."""
    import os
    import subprocess
    import sys
    from conftest import GOLDEN, ROOT
    paths = [os.path.join(GOLDEN, "jpeg", n + ".jpg") for n in ("bird_small", "tree_small")]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "sift-features_amd", "sift_match.py"), *paths,
                          "--processing", "opencv", "--ratio", "0.8"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    res = []
    for path in paths:
        with open(path, "rb") as f:
            res.append(ctx.sift_jpeg(f.read()))
    want = match_ref.match(res[1].descriptors, res[0].descriptors, 0.8, True)
    assert out.stdout.split("\n")[:3] == ["225 keypoints", "1270 keypoints", f"{len(want[0])} matches (ratio 0.8)"]


# ---- ABI (no device needed) ---------------------------------------------------------
def test_null_context_rejected(pkg):
    L = pkg.lib()
    buf = (ctypes.c_uint8 * 256)()
    n = ctypes.c_size_t()
    offs = (ctypes.c_size_t * 2)(0, 1)
    assert L.sift_mi_match_neighbors(None, buf, 1, buf, 1, buf) == -1
    assert L.sift_mi_match_ratio(None, buf, 1, buf, 1, 0.8, 1, buf, 1, ctypes.byref(n)) == -1
    assert L.sift_mi_match_pairs_device(None, buf, offs, 1, buf, 1, 0.8, 1, buf, 1, offs) == -1
    assert b"0.5.0" in L.sift_mi_version()
