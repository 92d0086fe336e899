"""Geometric verification of matched pairs on the GPU (sift_mi_verify_matches,
sift_mi_verify_pairs_device; csrc/verify.hip) against its numpy restatement
(verify_ref.py, pinned by test_verify_ref_cpu.py).  LABELLED EXTENSION: the
crate has nothing like it.

Without refits everything is bit-exact: h as bit patterns, the mask,
n_inliers, best_hypothesis.  With refits the masks, counts and accepted rounds
are equal, and the two H project the pair's query points to within 1e-3 px of
each other: one f32 ulp per entry of H on coordinates up to 640 px moves a
projection by about 5e-4 px, and the f64 solve behind it does not depend on
the order of its sums beyond that (test_refit_summation_order_and_lstsq).
The refit fixtures keep every match 1e-2 px from the threshold
(test_refit_fixtures_stay_clear_of_the_threshold), so that bound implies
equal masks."""
import ctypes
import functools

import numpy as np
import pytest
from conftest import load_golden

import match_ref
import verify_ref as V

gpu = pytest.mark.gpu

CHUNK = 1024  # csrc/sift_kernels.h kVerifyChunk: records of a pair in LDS at a time


def _arrays(rec):
    """A record list as two keypoint arrays and the identity matches."""
    rec = np.asarray(rec, np.float32).reshape(-1, 4)
    m = len(rec)
    kq, kt = np.zeros((m, 5), np.float32), np.zeros((m, 5), np.float32)
    kq[:, :2], kt[:, :2] = rec[:, :2], rec[:, 2:]
    i = np.arange(m, dtype=np.int32)
    return kq, kt, (i, i, np.zeros(m, np.float32))


def _gpu(ctx, rec, thr, it, seed, rounds):
    return ctx.verify_matches(*_arrays(rec), threshold=thr, iterations=it, seed=seed, refit_rounds=rounds)


def _assert_bit_exact(got, want, what=None):
    (H, mask, info), (rH, rmask, rinfo) = got, want
    assert info == rinfo, (what, info, rinfo)
    assert H.dtype == np.float32 and H.shape == (3, 3) and mask.dtype == bool
    assert np.array_equal(H.view(np.uint32), rH.view(np.uint32)), (what, H, rH)
    assert np.array_equal(mask, rmask), what
    assert info["n_inliers"] == mask.sum() <= info["n_matches"] == len(mask)


@functools.lru_cache(maxsize=None)
def _planted(m, seed):
    rec = V.planted(m, 0.6, seed)[0]
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def _ref(m, seed, it, rounds=0):
    return V.verify(_planted(m, seed), 2.0, it, seed, rounds)


# ---- bit-exact without refits ---------------------------------------------------
@gpu
@pytest.mark.parametrize("m", [0, 1, 3, 4, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2000])
def test_bit_exact_match_counts(ctx, m):
    """300 hypotheses: two workgroups per pair, the second partly filled."""
    got = _gpu(ctx, _planted(m, 100 + m), 2.0, 300, 100 + m, 0)
    _assert_bit_exact(got, _ref(m, 100 + m, 300), m)
    if m >= 63:
        assert got[2]["n_inliers"] > 0.5 * m  # the planted 60 %


@gpu
@pytest.mark.parametrize("it", [1, 255, 256, 257, 1024])
def test_bit_exact_iterations(ctx, it):
    _assert_bit_exact(_gpu(ctx, _planted(300, 9), 2.0, it, 9, 0), _ref(300, 9, it), it)


@gpu
def test_seed_changes_the_samples(ctx):
    a, b = _gpu(ctx, _planted(300, 9), 2.0, 64, 1, 0), _gpu(ctx, _planted(300, 9), 2.0, 64, 2, 0)
    assert a[2]["best_hypothesis"] != b[2]["best_hypothesis"] or not np.array_equal(a[0], b[0])
    _assert_bit_exact(b, V.verify(_planted(300, 9), 2.0, 64, 2, 0))
    _assert_bit_exact(_gpu(ctx, _planted(300, 9), 2.0, 64, 0xFFFFFFFF, 0), V.verify(_planted(300, 9), 2.0, 64, 0xFFFFFFFF, 0))


@gpu
@pytest.mark.parametrize("name", ["collinear", "duplicates"])
def test_no_model(ctx, name):
    rec = getattr(V, name)()
    for rounds in (0, 2):
        H, mask, info = _gpu(ctx, rec, 2.0, 256, 0, rounds)
        assert not H.any() and not mask.any()
        assert info == dict(n_matches=len(rec), n_inliers=0, best_hypothesis=-1, refits=0)
        _assert_bit_exact((H, mask, info), V.verify(rec, 2.0, 256, 0, rounds))


@gpu
def test_variant_fixtures(ctx):
    """The three fixtures on which test_verify_ref_cpu.py tells the wrong
    variants from the rule: the GPU gives the rule's answer, none of theirs."""
    rec = V.four()  # ties to the lowest hypothesis; sampling without replacement
    got = _gpu(ctx, rec, 2.0, 64, 0, 0)
    _assert_bit_exact(got, V.verify(rec, 2.0, 64, 0, 0))
    assert got[2]["best_hypothesis"] == 0 and got[2]["n_inliers"] == 4
    for v in ("tie_high", "repeat"):
        assert V.verify(rec, 2.0, 64, 0, 0, variant=v)[2]["best_hypothesis"] != 0
    rec = V.translation_exact()  # <= keeps the match displaced by exactly the threshold
    got = _gpu(ctx, rec, 2.0, 64, 0, 0)
    _assert_bit_exact(got, V.verify(rec, 2.0, 64, 0, 0))
    assert got[1].all() and np.array_equal(got[0], np.array([[1, 0, 5], [0, 1, -3], [0, 0, 1]], np.float32))
    assert not V.verify(rec, 2.0, 64, 0, 0, variant="thr_lt")[1][0]
    rec = V.square_swapped()  # the orientation test: no model
    got = _gpu(ctx, rec, 2.0, 64, 0, 0)
    _assert_bit_exact(got, V.verify(rec, 2.0, 64, 0, 0))
    assert got[2]["best_hypothesis"] == -1
    assert V.verify(rec, 2.0, 64, 0, 0, variant="no_orient")[2]["best_hypothesis"] == 0


# ---- segments ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    import torch
    kps, offs, pairs, matches, recs = V.segments()
    t = torch.from_numpy(kps.copy()).cuda()
    torch.cuda.synchronize()
    return t, kps, offs, pairs, matches, recs


@gpu
def test_segment_pairs(ctx, arena):
    t, kps, offs, pairs, matches, recs = arena
    assert len(pairs) == 10
    got = ctx.verify_pairs_device(t.data_ptr(), offs, pairs, matches, threshold=2.0, iterations=300, seed=5,
                                  refit_rounds=0)
    assert len(got) == len(pairs)
    for p, ((a, b), mt, rec, g) in enumerate(zip(pairs, matches, recs, got)):
        assert np.array_equal(V.records(kps[offs[a]:offs[a + 1]], kps[offs[b]:offs[b + 1]], mt), rec)
        assert g[2]["n_inliers"] <= g[2]["n_matches"] == len(rec)
        _assert_bit_exact(g, V.verify(rec, 2.0, 300, 5, 0), p)
        own = ctx.verify_matches(kps[offs[a]:offs[a + 1]], kps[offs[b]:offs[b + 1]], mt, threshold=2.0,
                                 iterations=300, seed=5, refit_rounds=0)
        _assert_bit_exact(g, own, p)
    _assert_bit_exact(got[V.SEG_TWICE], got[-1])  # the pair listed twice
    for p, m in enumerate(V.SEG_MATCHES):
        if m >= 64:
            assert got[p][2]["n_inliers"] > 0.5 * m


@gpu
@pytest.mark.parametrize("rounds", [1, 2])
def test_segment_pairs_refit(ctx, arena, rounds):
    """The same call with refits: every pair equals its own one-pair call bit
    for bit (the kernels are the same, and a pair's place is not an input),
    and the restatement in mask, counts and accepted rounds
    (test_segment_fixtures_stay_clear_of_the_threshold)."""
    t, kps, offs, pairs, matches, recs = arena
    got = ctx.verify_pairs_device(t.data_ptr(), offs, pairs, matches, threshold=2.0, iterations=300, seed=5,
                                  refit_rounds=rounds)
    for p, ((a, b), mt, rec, g) in enumerate(zip(pairs, matches, recs, got)):
        own = ctx.verify_matches(kps[offs[a]:offs[a + 1]], kps[offs[b]:offs[b + 1]], mt, threshold=2.0,
                                 iterations=300, seed=5, refit_rounds=rounds)
        _assert_bit_exact(g, own, p)
        rH, rmask, rinfo = V.verify(rec, 2.0, 300, 5, rounds)
        assert g[2] == rinfo and np.array_equal(g[1], rmask), (p, g[2], rinfo)
        assert g[2]["refits"] <= rounds and g[2]["n_inliers"] <= g[2]["n_matches"]
        if rinfo["best_hypothesis"] >= 0:
            assert np.abs(V.project(g[0], rec[:, :2]) - V.project(rH, rec[:, :2])).max() <= 1e-3


# ---- refit ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("rounds", [1, 2])
@pytest.mark.parametrize("m,share,seed", V.REFIT_CASES)
def test_refit(ctx, m, share, seed, rounds):
    rec, good = V.planted(m, share, seed)
    rH, rmask, rinfo = V.verify(rec, 2.0, 512, seed, rounds)
    H, mask, info = _gpu(ctx, rec, 2.0, 512, seed, rounds)
    d = np.abs(V.project(H, rec[:, :2]) - V.project(rH, rec[:, :2])).max()
    print(f"m {m} rounds {rounds}: refits {info['refits']} inliers {info['n_inliers']} (ref {rinfo['n_inliers']}), "
          f"projections differ by {d:.3g} px")
    assert info == rinfo
    assert np.array_equal(mask, rmask)
    assert d <= 1e-3
    assert info["refits"] >= 1 and (mask & good).sum() >= 0.95 * good.sum()


# ---- EINVAL ------------------------------------------------------------------------------
def _raw(pkg, ctx, d_ptr, offs, pairs, matches, po, prm, models=True, mask=True):
    from sift_features_amd import _lib
    L = pkg.lib()
    c_offs = None if offs is None else (ctypes.c_size_t * len(offs))(*[int(v) for v in offs])
    c_pairs = None if pairs is None else (_lib.SegPair * max(1, len(pairs)))(*[_lib.SegPair(a, b) for a, b in pairs])
    c_m = None if matches is None else (_lib.Match * max(1, len(matches)))(*[_lib.Match(q, t, 0.0) for q, t in matches])
    c_po = None if po is None else (ctypes.c_size_t * len(po))(*po)
    c_prm = None if prm is None else ctypes.byref(_lib.RansacParams(*prm))
    n_pairs = 0 if pairs is None else len(pairs)
    out = (_lib.Homography * max(1, n_pairs))() if models else None
    msk = (ctypes.c_uint8 * 64)() if mask else None
    return L.sift_mi_verify_pairs_device(ctx._h, ctypes.c_void_p(d_ptr), c_offs, 0 if offs is None else len(offs) - 1,
                                         c_pairs, n_pairs, c_m, c_po, c_prm, out, msk)


@gpu
def test_verify_einval(pkg, ctx):
    import torch
    rec = _planted(8, 1)
    kq, kt, _ = _arrays(rec)
    t = torch.from_numpy(np.concatenate([kq, kt])).cuda()
    torch.cuda.synchronize()
    d, offs, pairs, po, prm = t.data_ptr(), [0, 8, 16], [(0, 1)], [0, 8], (2.0, 64, 0, 1)
    mt = [(i, i) for i in range(8)]
    ok = lambda: _raw(pkg, ctx, d, offs, pairs, mt, po, prm)
    assert ok() == 0
    # a null argument
    assert _raw(pkg, ctx, None, offs, pairs, mt, po, prm) == -1
    assert _raw(pkg, ctx, d, None, pairs, mt, po, prm) == -1
    assert _raw(pkg, ctx, d, offs, None, mt, po, prm) == -1
    assert _raw(pkg, ctx, d, offs, pairs, None, po, prm) == -1
    assert _raw(pkg, ctx, d, offs, pairs, mt, None, prm) == -1
    assert _raw(pkg, ctx, d, offs, pairs, mt, po, None) == -1
    assert _raw(pkg, ctx, d, offs, pairs, mt, po, prm, models=False) == -1
    assert _raw(pkg, ctx, d, offs, pairs, mt, po, prm, mask=False) == -1
    # threshold: not finite, zero, negative
    for thr in (float("nan"), float("inf"), 0.0, -1.0):
        assert _raw(pkg, ctx, d, offs, pairs, mt, po, (thr, 64, 0, 1)) == -1, thr
        with pytest.raises(pkg.SiftMiError):
            ctx.verify_matches(kq, kt, (np.arange(8), np.arange(8)), threshold=thr)
    # iterations: 0, above 65536; refit_rounds above 8
    assert _raw(pkg, ctx, d, offs, pairs, mt, po, (2.0, 0, 0, 1)) == -1
    assert _raw(pkg, ctx, d, offs, pairs, mt, po, (2.0, 65537, 0, 1)) == -1
    assert _raw(pkg, ctx, d, offs, pairs, mt, po, (2.0, 64, 0, 9)) == -1
    assert _raw(pkg, ctx, d, offs, pairs, mt, po, (2.0, 64, 0, 8)) == 0
    # a pair index >= n_segs
    assert _raw(pkg, ctx, d, offs, [(0, 2)], mt, po, prm) == -1
    assert _raw(pkg, ctx, d, offs, [(2, 1)], mt, po, prm) == -1
    # decreasing offsets / pair_offsets
    assert _raw(pkg, ctx, d, [0, 10, 8], pairs, mt, po, prm) == -1
    assert _raw(pkg, ctx, d, offs, [(0, 1), (0, 1)], mt, [0, 8, 4], prm) == -1
    # a match index outside its pair's segment (either side, negative)
    for bad in ((8, 0), (0, 8), (-1, 0), (0, -1)):
        assert _raw(pkg, ctx, d, offs, pairs, mt[:7] + [bad], po, prm) == -1, bad
    assert b"segment" in pkg.lib().sift_mi_last_error()
    assert _raw(pkg, ctx, d, [0, 8, 15], pairs, mt, po, prm) == -1  # the train segment one row shorter
    # still usable afterwards, and no pairs at all is an empty result
    assert ok() == 0
    assert _raw(pkg, ctx, d, offs, [], mt, [0], prm) == 0
    _assert_bit_exact(ctx.verify_matches(kq, kt, (np.arange(8), np.arange(8)), 2.0, 64, 0, 0),
                      V.verify(rec, 2.0, 64, 0, 0))


# ---- end to end -----------------------------------------------------------------------------
@gpu
def test_verify_frames_end_to_end(pkg, ctx):
    """The three frames of test_match_frames_end_to_end: extraction, matching
    and verification without the keypoints leaving HBM; the restatement runs
    on the fetched keypoints."""
    import torch
    img = load_golden("bird_small")["image"]
    h, w = img.shape
    frames = np.stack([img, np.roll(img, 7, axis=1), np.roll(img, (5, -9), axis=(0, 1))])
    shifts = {(0, 1): (7, 0), (1, 2): (-16, 5), (0, 2): (-9, 5)}  # (dx, dy) of the pair's train frame
    host = ctx.sift_batch(frames)
    t = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    c2 = pkg.Context(0, pkg.OpenCVProcessing)
    try:
        offs, _ = c2.sift_batch_device(t.data_ptr(), 3, w, h, t.stride(1), t.stride(0), fetch=False)
        before = c2.device_results()
        pairs = list(shifts)
        matches = c2.match_frames(offs, pairs)
        got = c2.verify_frames(offs, pairs, matches)
        assert c2.device_results() == before  # only read
        pts = np.array([[w / 2, h / 2], [0, 0], [w - 1, h - 1]], np.float64)
        for (a, b), mt, (H, mask, info) in zip(pairs, matches, got):
            rec = V.records(host[a].keypoints_array, host[b].keypoints_array, mt)
            rH, rmask, rinfo = V.verify(rec, 3.0, 1024, 0, 2)
            dev = np.abs(V.project(H, pts) - (pts + shifts[a, b])).max()
            d = np.abs(V.project(H, rec[:, :2]) - V.project(rH, rec[:, :2])).max()
            print(f"pair {(a, b)}: {info} of ref {rinfo}; corners off the shift by {dev:.3g} px; "
                  f"projections differ by {d:.3g} px")
            assert V.near_threshold_any(rec, 3.0, 1024, 0, 2) == []
            assert info == rinfo and np.array_equal(mask, rmask) and d <= 1e-3
            assert info["n_inliers"] >= 200
            assert dev <= 0.25
    finally:
        c2.close()


@gpu
def test_sift_match_cli_verify(pkg, ctx):
    """sift_match.py --verify 3: the three lines of test_sift_match_cli, then
    the inlier count the restatement gives on the same matches."""
    import os
    import subprocess
    import sys
    from conftest import GOLDEN, ROOT
    paths = [os.path.join(GOLDEN, "jpeg", n + ".jpg") for n in ("bird_small", "tree_small")]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "sift-features_amd", "sift_match.py"), *paths,
                          "--processing", "opencv", "--ratio", "0.8", "--verify", "3"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    res = []
    for path in paths:
        with open(path, "rb") as f:
            res.append(ctx.sift_jpeg(f.read()))
    want = match_ref.match(res[1].descriptors, res[0].descriptors, 0.8, True)
    rec = V.records(res[1].keypoints_array, res[0].keypoints_array, want)
    info = V.verify(rec, 3.0, 1024, 0, 2)[2]
    print(out.stdout, info, V.near_threshold_any(rec, 3.0, 1024, 0, 2))
    assert V.near_threshold_any(rec, 3.0, 1024, 0, 2) == []
    assert out.stdout.split("\n")[:4] == ["225 keypoints", "1270 keypoints", f"{len(want[0])} matches (ratio 0.8)",
                                          f"{info['n_inliers']} inliers (homography, threshold 3)"]
