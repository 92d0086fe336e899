"""Feature tracks on the GPU (sift_mi_build_tracks_device; csrc/tracks.hip)
against their numpy restatement (tracks_ref.py, pinned by
test_tracks_ref_cpu.py), bit for bit in every output array: the computation
is integer, and obs' x, y are copied bit patterns.  LABELLED EXTENSION: the
crate has nothing like it.

Each fixture runs in the given order and with its pairs and matches permuted;
both results equal the restatement's, hence each other."""
import ctypes
import functools

import numpy as np
import pytest

import tracks_ref as T

gpu = pytest.mark.gpu

BAIT_ROWS = 16  # keypoint rows planted beyond offsets[n_segs]


def _raw(pkg, ctx, d_kps, c, min_length=2, drop=False, h=None):
    """The C entry point on input dict c.  Returns (rc, result dict or None);
    the output arrays carry the caller-provided sizes and a canary past them."""
    from sift_features_amd import _lib
    offs, po = c["offsets"], c["pair_offsets"]
    n = int(offs[-1] - offs[0])
    c_offs = (ctypes.c_size_t * len(offs))(*[int(v) for v in offs])
    c_po = (ctypes.c_size_t * len(po))(*[int(v) for v in po])
    pr = c["pairs"]
    c_pairs = (_lib.SegPair * max(len(pr), 1))(*[_lib.SegPair(a, b) for a, b in pr])
    rec = np.ascontiguousarray(c["matches"]) if len(c["matches"]) else np.zeros(1, T.MATCH)
    keep = c["keep"]
    track_of = np.full(n + 1, 12345, np.int32)
    t_offs = np.full(n // 2 + 3, 0xABCD, np.uint32)
    obs = np.zeros(n + 1, T.OBS)
    obs["seg"] = 0xABCD
    conflict = np.full(n // 2 + 2, 7, np.uint8)
    nt = ctypes.c_uint32(0xABCD)
    prm = _lib.TrackParams(min_length, 1 if drop else 0)
    rc = pkg.lib().sift_mi_build_tracks_device(
        ctx._h if h is None else h, ctypes.c_void_p(d_kps), c_offs, len(offs) - 1, c_pairs, len(pr), rec.ctypes.data,
        c_po, None if keep is None else np.ascontiguousarray(keep).ctypes.data, ctypes.byref(prm),
        track_of.ctypes.data, ctypes.byref(nt), t_offs.ctypes.data, obs.ctypes.data, conflict.ctypes.data)
    if rc != 0:
        return rc, None
    k = nt.value
    assert k <= n // 2
    # nothing past what the caller provides, nothing past what the result needs
    assert track_of[n] == 12345 and t_offs[n // 2 + 2] == 0xABCD and obs["seg"][n] == 0xABCD
    assert conflict[n // 2 + 1] == 7
    assert (t_offs[k + 1:] == 0xABCD).all() and (conflict[k:] == 7).all() and (obs["seg"][t_offs[k]:] == 0xABCD).all()
    return 0, dict(track_of=track_of[:n], offsets=t_offs[:k + 1], obs=obs[:int(t_offs[k])], conflict=conflict[:k])


@functools.lru_cache(maxsize=None)
def _arena(rows):
    """Device keypoints of `rows` rows and BAIT_ROWS more behind them."""
    import torch
    kps = T.keypoints(rows + BAIT_ROWS, seed=rows)
    kps.setflags(write=False)
    t = torch.from_numpy(kps.copy()).cuda()
    torch.cuda.synchronize()
    return t, kps


def _check(pkg, ctx, c, what=None, **kw):
    """c in the given and in a permuted order against the restatement."""
    t, kps = _arena(int(c["offsets"][-1]))
    want = T.run(c, kps=kps, min_length=kw.get("min_length", 2), drop_conflicts=kw.get("drop", False))
    for cc in (c, T.permuted(c, 1)):
        rc, got = _raw(pkg, ctx, t.data_ptr(), cc, **kw)
        assert rc == 0, pkg.lib().sift_mi_last_error()
        for key in ("track_of", "offsets", "conflict"):
            assert np.array_equal(got[key], want[key]), (what, key)
        assert got["obs"].tobytes() == want["obs"].tobytes(), what
    return want


def _split(n, k):
    """n rows over k segments, the first ones the larger."""
    return [n // k + (1 if i < n % k else 0) for i in range(k)]


# ---- row counts around the wave and workgroup sizes --------------------------------
@gpu
@pytest.mark.parametrize("n,k", [(1, 1), (63, 2), (64, 3), (65, 4), (255, 5), (256, 2), (257, 3)])
def test_row_counts(pkg, ctx, n, k):
    c = T.random_graph(_split(n, k), 2 * k + 1, 0.35, seed=n, keep_share=0.9)
    want = _check(pkg, ctx, c, n)
    _check(pkg, ctx, c, n, min_length=3, drop=True)
    if n >= 63:
        assert len(want["offsets"]) > 2 and want["conflict"].any() and not want["conflict"].all()


@gpu
def test_path_of_128_segments_supplied_last_to_first(pkg, ctx):
    """One keypoint per frame; every pair's link re-links the root of the one before."""
    want = _check(pkg, ctx, T.chain(128, reverse=True))
    assert want["offsets"].tolist() == [0, 128] and want["conflict"].tolist() == [0]
    assert want["obs"]["seg"].tolist() == list(range(128))


@gpu
def test_hub_4096_matches_on_one_row(pkg, ctx):
    """Maximal contention on one CAS target: the hub is the largest row, so
    all 4096 lanes try to link parent[4096] and the losers retry on the
    winner (tracks_ref.hub).  In the given order, permuted (_check) and with
    every match four times."""
    want = _check(pkg, ctx, T.hub(4096))
    assert want["offsets"].tolist() == [0, 4097] and want["conflict"].tolist() == [1]
    assert want["track_of"].tolist() == [0] * 4097
    _check(pkg, ctx, T.hub(4096), drop=True)
    c = T.hub(4096)
    four = T.case([4096, 1], [(0, 1)] * 4, [(c["matches"]["query_idx"], c["matches"]["train_idx"])] * 4)
    assert T.equal(_check(pkg, ctx, four), want)


@gpu
def test_star_4096_matches_from_the_smallest_row(pkg, ctx):
    """The centre is row 0: every link has a cell of its own."""
    want = _check(pkg, ctx, T.star(4096))
    assert want["offsets"].tolist() == [0, 4097] and want["conflict"].tolist() == [1]


@gpu
def test_one_row_through_the_device(pkg, ctx):
    """N = 1 with a kept self edge: every kernel runs on one row; no track."""
    want = _check(pkg, ctx, T.case([1], [(0, 0)], [([0], [0])]))
    assert want["track_of"].tolist() == [-1] and want["offsets"].tolist() == [0]
    want = _check(pkg, ctx, T.case([0, 1, 0], [(1, 1), (1, 1)], [([0, 0], [0, 0]), ([0], [0])], base=7))
    assert want["track_of"].tolist() == [-1]


@functools.lru_cache(maxsize=None)
def _two_components():
    """Two random trees of 10 000 rows (segments 0, 1 and 2, 3), joined by the last match."""
    rng = np.random.default_rng(5)
    half = 5000
    per = []
    for _ in range(2):  # keypoint i of the second segment hangs under a random earlier row of the pair
        up = np.array([rng.integers(0, half + i) for i in range(half)])
        chain = (np.arange(1, half), np.arange(half - 1))  # the first segment: a path, by a self pair
        per += [chain, (up[up < half], np.nonzero(up < half)[0]), (up[up >= half] - half, np.nonzero(up >= half)[0])]
    pairs = [(0, 0), (0, 1), (1, 1), (2, 2), (2, 3), (3, 3), (1, 2)]
    per.append(([half - 1], [0]))
    return T.case([half] * 4, pairs, per)


@gpu
@pytest.mark.parametrize("joined", [True, False])
def test_two_large_components_and_the_match_between_them(pkg, ctx, joined):
    c = dict(_two_components())
    total = len(c["matches"])
    c["keep"] = np.ones(total, np.uint8)
    c["keep"][-1] = joined
    t, kps = _arena(20000)
    want = T.run(c, kps=kps)
    assert np.diff(want["offsets"].astype(np.int64)).tolist() == ([20000] if joined else [10000, 10000])
    rc, got = _raw(pkg, ctx, t.data_ptr(), c)
    assert rc == 0 and T.equal(got, want)
    rc, got = _raw(pkg, ctx, t.data_ptr(), T.permuted(c, 2))
    assert rc == 0 and T.equal(got, want)


# ---- conflicts, self pairs, duplicates, short components -------------------------
@gpu
@pytest.mark.parametrize("drop", [False, True])
def test_conflicts_self_pairs_and_duplicates(pkg, ctx, drop):
    for name in ("conflict_ends", "keep_ignored", "first_appearance", "min_length_edges"):
        _check(pkg, ctx, T.FIXTURES[name], name, drop=drop)
    # a self pair with a match of a row to itself, and duplicate matches
    c = T.case([3, 2], [(0, 0), (0, 1), (0, 1)], [([1, 2], [1, 0]), ([0], [1]), ([0], [1])], base=40)
    want = _check(pkg, ctx, c, "self", drop=drop)
    assert want["track_of"].tolist() == ([-1] * 5 if drop else [0, -1, 0, -1, 0])
    c = T.case([4, 4], [(0, 1)], [([0, 0, 0, 1, 1], [2, 2, 2, 3, 3])])
    assert _check(pkg, ctx, c, "duplicates", drop=drop)["offsets"].tolist() == [0, 2, 4]


@gpu
@pytest.mark.parametrize("min_length", [2, 3, 8])
def test_min_length(pkg, ctx, min_length):
    c = T.chain(7, per_seg=5)  # five components of 7 rows
    c["keep"] = np.ones(len(c["matches"]), np.uint8)
    c["keep"][[5, 11, 17]] = 0  # ... three of them cut: 2 + 5, 3 + 4, 4 + 3
    want = _check(pkg, ctx, c, min_length=min_length)
    sizes = np.diff(T.run(c)["offsets"].astype(np.int64))
    assert sorted(sizes.tolist()) == [2, 3, 3, 4, 4, 5, 7, 7]
    assert len(want["offsets"]) - 1 == int((sizes >= min_length).sum())
    if min_length == 8:
        assert len(want["offsets"]) == 1 and (want["track_of"] == -1).all()


# ---- bounds ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("drop", [False, True])
def test_segment_arena_with_bait(pkg, ctx, drop):
    """Empty segments, empty pairs, offsets[0] != 0, matches planted before
    pair_offsets[0] and after pair_offsets[n_pairs] that would merge tracks,
    keypoints planted beyond offsets[n_segs] (_arena)."""
    c = T.random_graph(T.SEG_LENS, 16, 0.3, 5, base=11, keep_share=0.8)
    c["pairs"] += [(0, 7), (2, 0)]  # pairs of empty segments: no matches
    c["pair_offsets"] = np.append(c["pair_offsets"], [c["pair_offsets"][-1]] * 2)
    plain = T.run(c, drop_conflicts=drop)
    b = T.with_bait(c, 5, 5)
    assert not T.equal(T.run(b, variant="read_outside", drop_conflicts=drop), plain)
    want = _check(pkg, ctx, b, "bait", drop=drop)
    for key in ("track_of", "offsets", "conflict"):  # the bait changed nothing
        assert np.array_equal(want[key], plain[key]), key
    assert len(want["offsets"]) > 10
    for name in ("read_outside", "no_seg_base", "train_on_query"):
        _check(pkg, ctx, T.FIXTURES[name], name, drop=drop)


@gpu
def test_more_segments_than_the_lds_table(pkg, ctx):
    """2049+ segment starts: k_track_init searches them in global memory."""
    lens = [1, 0, 2] * 700  # 2100 segments, 2100 rows
    rng = np.random.default_rng(8)
    live = [s for s, n in enumerate(lens) if n]
    pairs = [(live[i], live[j]) for i, j in rng.integers(0, len(live), (300, 2))]
    c = T.case(lens, pairs, [([lens[a] - 1], [0]) for a, b in pairs])
    assert len(_check(pkg, ctx, c)["offsets"]) > 50


@gpu
def test_obs_are_the_keypoints_bit_patterns(pkg, ctx):
    c = T.chain(3, per_seg=4)
    t, kps = _arena(12)
    want = _check(pkg, ctx, c)
    rows = want["obs"]["seg"] * 4 + want["obs"]["idx"]
    assert np.array_equal(want["obs"]["x"].view(np.uint32), kps[rows, 0].view(np.uint32))
    assert np.isnan(kps[1, 0]) and np.signbit(kps[2, 1])  # a NaN and a -0.0 among them


# ---- empty inputs --------------------------------------------------------------------------
@gpu
def test_empty_inputs(pkg, ctx):
    for c in (T.case([5, 4], [], []),                                  # no pairs
              T.case([5, 4], [(0, 1), (1, 0)], [([], []), ([], [])]),  # no matches
              T.case([5, 4], [(0, 1)], [([0, 1], [0, 1])], keep=[0, 0]),  # keep all zero
              T.case([0, 0], [(0, 1)], [([], [])]),                    # N == 0
              T.case([], [], [])):
        want = _check(pkg, ctx, c)
        assert want["offsets"].tolist() == [0] and (want["track_of"] == -1).all()


# ---- EINVAL ------------------------------------------------------------------------------------
@gpu
def test_invalid_arguments_leave_the_device_results(pkg, ctx, synth):
    import torch
    img = synth.frame(160, 120, 3)
    frames = np.stack([img, np.roll(img, 5, axis=1)])
    ft = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    c2 = pkg.Context(0, pkg.OpenCVProcessing)
    try:
        offs, _ = c2.sift_batch_device(ft.data_ptr(), 2, 160, 120, ft.stride(1), ft.stride(0), fetch=False)
        before = c2.device_results()
        n0, n1 = int(offs[1] - offs[0]), int(offs[2] - offs[1])
        assert n0 > 4 and n1 > 4
        good = T.case([n0, n1], [(0, 1)], [([0, 1], [1, 0])])
        bad = {}
        bad["min_length"] = (good, dict(min_length=1))
        bad["pair index"] = (dict(good, pairs=[(0, 2)]), {})
        bad["offsets decrease"] = (dict(good, offsets=np.array([0, n0 + n1, n0])), {})
        bad["pair_offsets decrease"] = (dict(good, pairs=[(0, 1), (1, 0)], pair_offsets=np.array([0, 2, 1])), {})
        for q, t in ((n0, 0), (0, n1), (-1, 0), (0, -1)):
            bad[f"match {q, t}"] = (dict(good, matches=T.records([0, q], [0, t])), {})
        counters = c2.track_counters()
        for what, (c, kw) in bad.items():
            rc, _ = _raw(pkg, c2, before[0], c, h=c2._h, **kw)
            assert rc == -1, what
            assert c2.device_results() == before, what
            assert c2.track_counters() == counters, what  # no device work
        # more than 2^31 - 1 rows / matches: only the tables say so, nothing is read
        huge = dict(good, offsets=np.array([0, 1 << 31, (1 << 31) + 1]), pairs=[], pair_offsets=np.array([0]),
                    matches=T.records([], []))
        from sift_features_amd import _lib
        L = pkg.lib()
        one = (ctypes.c_uint8 * 64)()
        nt = ctypes.c_uint32()
        prm = _lib.TrackParams(2, 0)
        o3 = (ctypes.c_size_t * 3)(*[int(v) for v in huge["offsets"]])
        p1 = (ctypes.c_size_t * 1)(0)
        assert L.sift_mi_build_tracks_device(c2._h, ctypes.c_void_p(before[0]), o3, 2, one, 0, one, p1, None,
                                             ctypes.byref(prm), one, ctypes.byref(nt), one, one, one) == -1
        assert b"2^31" in L.sift_mi_last_error()
        o2 = (ctypes.c_size_t * 2)(0, 0)
        p2 = (ctypes.c_size_t * 2)(0, 1 << 31)
        pair = _lib.SegPair(0, 0)
        assert L.sift_mi_build_tracks_device(c2._h, ctypes.c_void_p(before[0]), o2, 1, ctypes.byref(pair), 1, one, p2,
                                             None, ctypes.byref(prm), one, ctypes.byref(nt), one, one, one) == -1
        assert b"2^31" in L.sift_mi_last_error()
        assert c2.device_results() == before
        # and the valid call still runs on them
        got = c2.track_frames(offs, [(0, 1)], [(np.array([0, 1]), np.array([1, 0]))])
        assert len(got) == 2 and c2.device_results() == before
    finally:
        c2.close()


# ---- the Python interface --------------------------------------------------------------------
@gpu
def test_python_interface(pkg, ctx):
    c = T.panning(6, 70, 2)
    t, kps = _arena(int(c["offsets"][-1]))
    po = c["pair_offsets"]
    m = c["matches"]
    triples = [(m["query_idx"][po[p]:po[p + 1]], m["train_idx"][po[p]:po[p + 1]], m["distance"][po[p]:po[p + 1]])
               for p in range(len(c["pairs"]))]
    keep = [c["keep"][po[p]:po[p + 1]].astype(bool) for p in range(len(c["pairs"]))]
    ctx.reset_stats()
    for conflicts in ("flag", "drop"):
        want = T.run(c, kps=kps, min_length=3, drop_conflicts=conflicts == "drop")
        got = ctx.build_tracks_device(t.data_ptr(), c["offsets"], c["pairs"], triples, keep, min_length=3,
                                      conflicts=conflicts)
        assert isinstance(got, pkg.Tracks) and len(got) == len(want["offsets"]) - 1 > 0
        assert got.track_of.dtype == np.int32 and np.array_equal(got.track_of, want["track_of"])
        assert np.array_equal(got.offsets, want["offsets"]) and got.obs.tobytes() == want["obs"].tobytes()
        assert got.conflict.dtype == bool and np.array_equal(got.conflict, want["conflict"].astype(bool))
        assert got.members(0).tobytes() == want["obs"][:want["offsets"][1]].tobytes()
        with pytest.raises(IndexError):
            got.members(len(got))
    # verify-style tuples as keep, and no keep at all
    tup = [(None, k, {}) for k in keep]
    assert np.array_equal(ctx.build_tracks_device(t.data_ptr(), c["offsets"], c["pairs"], triples, tup).track_of,
                          T.run(c)["track_of"])
    assert np.array_equal(ctx.build_tracks_device(t.data_ptr(), c["offsets"], c["pairs"], triples).track_of,
                          T.run(dict(c, keep=None))["track_of"])
    with pytest.raises(ValueError):
        ctx.build_tracks_device(t.data_ptr(), c["offsets"], c["pairs"], triples, conflicts="split")
    with pytest.raises(ValueError):
        ctx.track_frames(c["offsets"], c["pairs"], triples, conflicts="split")
    with pytest.raises(pkg.SiftMiError):
        ctx.build_tracks_device(t.data_ptr(), c["offsets"], c["pairs"], triples, min_length=1)
    counters = ctx.track_counters()
    assert counters["kernel_ms"] > 0
    assert counters["edges"] == 2 * int(c["keep"].sum()) + int(c["keep"].sum()) + len(m)
    ctx.reset_stats()
    assert ctx.track_counters() == {"kernel_ms": 0.0, "edges": 0}


# ---- end to end ---------------------------------------------------------------------------------
@gpu
def test_track_frames_end_to_end(pkg, ctx, synth):
    """Extraction, matching, verification and the tracks without the
    keypoints leaving HBM; the restatement runs on the fetched arrays."""
    import torch
    img = synth.frame(320, 213, 7)
    frames = np.stack([img, np.roll(img, 7, axis=1), np.roll(img, (5, -9), axis=(0, 1))])
    host = ctx.sift_batch(frames)
    t = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    c2 = pkg.Context(0, pkg.OpenCVProcessing)
    try:
        offs, _ = c2.sift_batch_device(t.data_ptr(), 3, 320, 213, t.stride(1), t.stride(0), fetch=False)
        before = c2.device_results()
        pairs = [(0, 1), (1, 2), (0, 2)]
        matches = c2.match_frames(offs, pairs, ratio=0.8)
        verified = c2.verify_frames(offs, pairs, matches)
        kps = np.concatenate([r.keypoints_array for r in host])
        c = T.case([len(r) for r in host], pairs, [(m[0], m[1]) for m in matches],
                   keep=np.concatenate([v[1] for v in verified]).astype(np.uint8))
        assert np.array_equal(c["offsets"], np.asarray(offs, np.int64))
        for conflicts, min_length in (("flag", 2), ("drop", 3)):
            got = c2.track_frames(offs, pairs, matches, keep=verified, min_length=min_length, conflicts=conflicts)
            assert c2.device_results() == before  # only read
            want = T.run(c, kps=kps, min_length=min_length, drop_conflicts=conflicts == "drop")
            print(f"{conflicts}, min_length {min_length}: {len(got)} tracks, {len(got.obs)} observations, "
                  f"{int(got.conflict.sum())} in conflict")
            assert len(got) > (8 if conflicts == "flag" else 0)
            assert np.array_equal(got.track_of, want["track_of"]) and np.array_equal(got.offsets, want["offsets"])
            assert got.obs.tobytes() == want["obs"].tobytes()
            assert np.array_equal(got.conflict, want["conflict"].astype(bool))
        assert (np.diff(got.offsets.astype(np.int64)) == 3).all()  # three frames, no conflicts: every track has one of each
    finally:
        c2.close()
