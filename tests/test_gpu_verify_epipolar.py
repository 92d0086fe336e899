"""Epipolar verification of matched pairs on the GPU
(sift_mi_verify_matches_epipolar, sift_mi_verify_pairs_epipolar_device;
csrc/verify_epipolar.hip) against its numpy restatement (epipolar_ref.py,
pinned by test_epipolar_ref_cpu.py).  LABELLED EXTENSION: the crate has
nothing like it.

Without refits everything is bit-exact: F as bit patterns, the mask,
n_inliers, best_hypothesis.  With refits the masks, counts and accepted rounds
are equal, and the f64 Sampson distances of all the pair's matches under the
two F differ by at most 1e-3 px: one f32 ulp per entry of F moves an inlier's
Sampson distance by up to 1.3e-4 px at 640 px, and the f64 eigen-solve behind
it does not depend on the order of its sums beyond that
(test_refit_summation_order).  The refit fixtures keep every match 1e-2 px
from the threshold (test_refit_fixtures_stay_clear_of_the_threshold), so that
bound implies equal masks."""
import ctypes
import functools

import numpy as np
import pytest
from conftest import load_golden

import epipolar_ref as E
import match_ref
import verify_ref as V

gpu = pytest.mark.gpu

CHUNK = 1024  # csrc/sift_kernels.h kVerifyChunk: records of a pair in LDS at a time
NONE = dict(n_inliers=0, best_hypothesis=-1, refits=0)


def _arrays(rec):
    """A record list as two keypoint arrays and the identity matches."""
    rec = np.asarray(rec, np.float32).reshape(-1, 4)
    m = len(rec)
    kq, kt = np.zeros((m, 5), np.float32), np.zeros((m, 5), np.float32)
    kq[:, :2], kt[:, :2] = rec[:, :2], rec[:, 2:]
    i = np.arange(m, dtype=np.int32)
    return kq, kt, (i, i, np.zeros(m, np.float32))


def _gpu(ctx, rec, thr, it, seed, rounds):
    return ctx.verify_matches(*_arrays(rec), threshold=thr, iterations=it, seed=seed, refit_rounds=rounds,
                              model="fundamental")


def _assert_bit_exact(got, want, what=None):
    (F, mask, info), (rF, rmask, rinfo) = got, want
    assert info == rinfo, (what, info, rinfo)
    assert F.dtype == np.float32 and F.shape == (3, 3) and mask.dtype == bool
    assert np.array_equal(F.view(np.uint32), rF.view(np.uint32)), (what, F, rF)
    assert np.array_equal(mask, rmask), what
    assert info["n_inliers"] == mask.sum() <= info["n_matches"] == len(mask)


def _assert_refit_equal(got, want, rec, what=None):
    """With refits: info and mask equal, Sampson distances of all matches within 1e-3 px."""
    (F, mask, info), (rF, rmask, rinfo) = got, want
    assert info == rinfo, (what, info, rinfo)
    assert np.array_equal(mask, rmask), what
    if rinfo["best_hypothesis"] < 0:
        assert not F.any()
        return 0.0
    a, b = E.sampson(rec, F), E.sampson(rec, rF)
    d = float(np.abs(a - b).max())
    assert d <= 1e-3, (what, d)
    return d


@functools.lru_cache(maxsize=None)
def _planted(m, seed):
    rec = E.planted(m, 0.6, seed)[0]
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def _ref(m, seed, it, rounds=0):
    return E.verify(_planted(m, seed), 2.0, it, seed, rounds)


# ---- bit-exact without refits ---------------------------------------------------
@gpu
@pytest.mark.parametrize("m", [0, 1, 7, 8, 9, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2000])
def test_bit_exact_match_counts(ctx, m):
    """300 hypotheses: two scoring workgroups per pair, the second partly filled (five of the models kernel)."""
    got = _gpu(ctx, _planted(m, 100 + m), 2.0, 300, 100 + m, 0)
    _assert_bit_exact(got, _ref(m, 100 + m, 300), m)
    if m < 8:
        assert got[2] == dict(n_matches=m, **NONE) and not got[0].any()
    else:
        assert np.abs(got[0]).max() == 1.0 and got[2]["best_hypothesis"] >= 0
    if m >= 63:
        assert got[2]["n_inliers"] > 0.5 * m  # the planted 60 %


@gpu
@pytest.mark.parametrize("it", [1, 255, 256, 257, 1024])
def test_bit_exact_iterations(ctx, it):
    _assert_bit_exact(_gpu(ctx, _planted(300, 9), 2.0, it, 9, 0), _ref(300, 9, it), it)


@gpu
def test_seed_changes_the_samples(ctx):
    rec = _planted(300, 9)
    got = {seed: _gpu(ctx, rec, 2.0, 64, seed, 0) for seed in (1, 2, 0xFFFFFFFF)}
    assert got[1][2]["best_hypothesis"] != got[2][2]["best_hypothesis"] or not np.array_equal(got[1][0], got[2][0])
    for seed, g in got.items():
        _assert_bit_exact(g, E.verify(rec, 2.0, 64, seed, 0), seed)


@gpu
def test_no_model(ctx):
    """Every match the same point pair: equal rows, an exact zero pivot in every sample."""
    rec = V.duplicates()
    for rounds in (0, 2):
        F, mask, info = _gpu(ctx, rec, 2.0, 256, 0, rounds)
        assert not F.any() and not mask.any()
        assert info == dict(n_matches=len(rec), **NONE)
        _assert_bit_exact((F, mask, info), E.verify(rec, 2.0, 256, 0, rounds))
    for m in range(8):
        F, mask, info = _gpu(ctx, _planted(64, 1)[:m], 2.0, 64, 0, 2)
        assert not F.any() and not mask.any() and info == dict(n_matches=m, **NONE)


@gpu
def test_variant_fixtures(ctx):
    """The fixtures on which test_epipolar_ref_cpu.py tells the wrong variants
    from the rule: the GPU gives the rule's answer, none of theirs."""
    rec = E.eight_exact()  # ties to the lowest hypothesis; sampling without replacement
    got = _gpu(ctx, rec, 2.0, 64, 0, 0)
    _assert_bit_exact(got, E.verify(rec, 2.0, 64, 0, 0))
    assert got[2]["best_hypothesis"] == 0 and got[2]["n_inliers"] == 8
    for v in ("tie_high", "repeat"):
        assert E.verify(rec, 2.0, 64, 0, 0, variant=v)[2]["best_hypothesis"] != 0
    rec = E.threshold_exact()  # <= keeps the match exactly on the threshold; both gradients in d
    got = _gpu(ctx, rec, 3.0, 64, 0, 0)
    _assert_bit_exact(got, E.verify(rec, 3.0, 64, 0, 0))
    assert got[1].all() and np.array_equal(got[0], np.array([[0, 0, 0], [0, 0, -0.75], [0, 1, 0]], np.float32))
    for v in ("thr_lt", "one_sided"):
        assert not E.verify(rec, 3.0, 64, 0, 0, variant=v)[1][0]
    rec = E.sideways()  # f[8] == 0: the column pivoting
    got = _gpu(ctx, rec, 2.0, 64, 0, 0)
    _assert_bit_exact(got, E.verify(rec, 2.0, 64, 0, 0))
    assert got[2]["best_hypothesis"] == 0 and got[2]["n_inliers"] == 40 and got[0][2, 2] == 0
    assert E.verify(rec, 2.0, 64, 0, 0, variant="no_colpivot")[2]["best_hypothesis"] != 0


# ---- segments ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    import torch
    kps, offs, pairs, matches, recs = E.segments()
    t = torch.from_numpy(kps.copy()).cuda()
    torch.cuda.synchronize()
    return t, kps, offs, pairs, matches, recs


@functools.lru_cache(maxsize=None)
def _seg_ref(p, rounds):
    return E.verify(E.segments()[4][p], 2.0, 300, 5, rounds)


@gpu
def test_segment_pairs(ctx, arena):
    t, kps, offs, pairs, matches, recs = arena
    assert len(pairs) == 10
    got = ctx.verify_pairs_device(t.data_ptr(), offs, pairs, matches, threshold=2.0, iterations=300, seed=5,
                                  refit_rounds=0, model="fundamental")
    assert len(got) == len(pairs)
    for p, ((a, b), mt, rec, g) in enumerate(zip(pairs, matches, recs, got)):
        assert g[2]["n_inliers"] <= g[2]["n_matches"] == len(rec)
        _assert_bit_exact(g, _seg_ref(p, 0), p)
        own = ctx.verify_matches(kps[offs[a]:offs[a + 1]], kps[offs[b]:offs[b + 1]], mt, threshold=2.0,
                                 iterations=300, seed=5, refit_rounds=0, model="fundamental")
        _assert_bit_exact(g, own, p)
    _assert_bit_exact(got[E.SEG_TWICE], got[-1])  # the pair listed twice
    for p, m in enumerate(E.SEG_MATCHES):
        if m >= 64:
            assert got[p][2]["n_inliers"] > 0.5 * m
        if m < 8:
            assert got[p][2] == dict(n_matches=m, **NONE)


@gpu
@pytest.mark.parametrize("rounds", [1, 2])
def test_segment_pairs_refit(ctx, arena, rounds):
    """The same call with refits: every pair equals its own one-pair call bit
    for bit (the kernels are the same, and a pair's place is not an input),
    and the restatement in mask, counts and accepted rounds
    (test_segment_fixtures_stay_clear_of_the_threshold)."""
    t, kps, offs, pairs, matches, recs = arena
    got = ctx.verify_pairs_device(t.data_ptr(), offs, pairs, matches, threshold=2.0, iterations=300, seed=5,
                                  refit_rounds=rounds, model="fundamental")
    for p, ((a, b), mt, rec, g) in enumerate(zip(pairs, matches, recs, got)):
        own = ctx.verify_matches(kps[offs[a]:offs[a + 1]], kps[offs[b]:offs[b + 1]], mt, threshold=2.0,
                                 iterations=300, seed=5, refit_rounds=rounds, model="fundamental")
        _assert_bit_exact(g, own, p)
        d = _assert_refit_equal(g, _seg_ref(p, rounds), rec, p)
        print(f"pair {p} m {len(rec)} rounds {rounds}: {g[2]}, Sampson distances differ by {d:.3g} px")
        assert g[2]["refits"] <= rounds and g[2]["n_inliers"] <= g[2]["n_matches"]
        if len(rec) >= 64:
            assert g[2]["refits"] >= 1
    _assert_bit_exact(got[E.SEG_TWICE], got[-1])


# ---- refit ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("rounds", [1, 2])
@pytest.mark.parametrize("m,share,seed", E.REFIT_CASES)
def test_refit(ctx, m, share, seed, rounds):
    rec, good = E.planted(m, share, seed)
    want = E.verify(rec, 2.0, 512, seed, rounds)
    got = _gpu(ctx, rec, 2.0, 512, seed, rounds)
    F, mask, info = got
    print(f"m {m} rounds {rounds}: {info} (ref {want[2]})")
    d = _assert_refit_equal(got, want, rec)
    s = np.linalg.svd(F.astype(np.float64), compute_uv=False)
    print(f"Sampson distances differ by {d:.3g} px; sigma3 / sigma1 {s[2] / s[0]:.3g}")
    assert info["refits"] >= 1 and (mask & good).sum() >= 0.95 * good.sum()
    assert s[2] / s[0] < 1e-6  # rank 2 after an accepted refit


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
    out = (_lib.Fundamental * max(1, n_pairs))() if models else None
    msk = (ctypes.c_uint8 * 64)() if mask else None
    return L.sift_mi_verify_pairs_epipolar_device(ctx._h, ctypes.c_void_p(d_ptr), c_offs,
                                                  0 if offs is None else len(offs) - 1, c_pairs, n_pairs, c_m, c_po,
                                                  c_prm, out, msk)


@gpu
def test_verify_einval(pkg, ctx):
    import torch
    from sift_features_amd import _lib
    rec = _planted(16, 1)
    kq, kt, ident = _arrays(rec)
    t = torch.from_numpy(np.concatenate([kq, kt])).cuda()
    torch.cuda.synchronize()
    d, offs, pairs, po, prm = t.data_ptr(), [0, 16, 32], [(0, 1)], [0, 16], (2.0, 64, 0, 1)
    mt = [(i, i) for i in range(16)]
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
    L = pkg.lib()
    c_m = (_lib.Match * 16)(*[_lib.Match(i, i, 0.0) for i in range(16)])
    one = lambda model, params: L.sift_mi_verify_matches_epipolar(
        ctx._h, kq.ctypes.data, 16, kt.ctypes.data, 16, c_m, 16, params, model, (ctypes.c_uint8 * 16)())
    assert one(ctypes.byref(_lib.Fundamental()), ctypes.byref(_lib.RansacParams(*prm))) == 0
    assert one(None, ctypes.byref(_lib.RansacParams(*prm))) == -1
    assert one(ctypes.byref(_lib.Fundamental()), None) == -1
    # threshold: not finite, zero, negative
    for thr in (float("nan"), float("inf"), 0.0, -1.0):
        assert _raw(pkg, ctx, d, offs, pairs, mt, po, (thr, 64, 0, 1)) == -1, thr
        with pytest.raises(pkg.SiftMiError):
            ctx.verify_matches(kq, kt, ident, threshold=thr, model="fundamental")
    # iterations: 0, above 65536; refit_rounds above 8
    assert _raw(pkg, ctx, d, offs, pairs, mt, po, (2.0, 0, 0, 1)) == -1
    assert _raw(pkg, ctx, d, offs, pairs, mt, po, (2.0, 65537, 0, 1)) == -1
    assert _raw(pkg, ctx, d, offs, pairs, mt, po, (2.0, 64, 0, 9)) == -1
    assert _raw(pkg, ctx, d, offs, pairs, mt, po, (2.0, 64, 0, 8)) == 0
    # a pair index >= n_segs
    assert _raw(pkg, ctx, d, offs, [(0, 2)], mt, po, prm) == -1
    assert _raw(pkg, ctx, d, offs, [(2, 1)], mt, po, prm) == -1
    # decreasing offsets / pair_offsets
    assert _raw(pkg, ctx, d, [0, 20, 16], pairs, mt, po, prm) == -1
    assert _raw(pkg, ctx, d, offs, [(0, 1), (0, 1)], mt, [0, 16, 8], prm) == -1
    # a match index outside its pair's segment (either side, negative)
    for bad in ((16, 0), (0, 16), (-1, 0), (0, -1)):
        assert _raw(pkg, ctx, d, offs, pairs, mt[:15] + [bad], po, prm) == -1, bad
    assert b"segment" in pkg.lib().sift_mi_last_error()
    assert _raw(pkg, ctx, d, [0, 16, 31], pairs, mt, po, prm) == -1  # the train segment one row shorter
    # an unknown model is refused before anything runs
    for call in (lambda: ctx.verify_matches(kq, kt, ident, model="nonsense"),
                 lambda: ctx.verify_pairs_device(d, offs, pairs, [ident], model="nonsense"),
                 lambda: ctx.verify_frames(offs, pairs, [ident], model="nonsense"),
                 lambda: pkg.verify_matches(kq, kt, ident, model="nonsense")):
        with pytest.raises(ValueError):
            call()
    # still usable afterwards, and no pairs at all is an empty result
    assert ok() == 0
    assert _raw(pkg, ctx, d, offs, [], mt, [0], prm) == 0
    _assert_bit_exact(ctx.verify_matches(kq, kt, ident, 2.0, 64, 0, 0, model="fundamental"),
                      E.verify(rec, 2.0, 64, 0, 0))


# ---- the homography path is untouched ------------------------------------------------------
@gpu
def test_homography_is_the_default(ctx):
    rec = V.planted(300, 0.6, 9)[0]
    want = V.verify(rec, 2.0, 300, 9, 0)
    for kw in ({}, {"model": "homography"}):
        H, mask, info = ctx.verify_matches(*_arrays(rec), threshold=2.0, iterations=300, seed=9, refit_rounds=0, **kw)
        assert info == want[2] and np.array_equal(mask, want[1])
        assert np.array_equal(H.view(np.uint32), want[0].view(np.uint32)) and H[2, 2] == 1.0


# ---- end to end -----------------------------------------------------------------------------
@gpu
def test_verify_frames_end_to_end(pkg, ctx):
    """The three rolled frames of test_gpu_verify.py's end-to-end test:
    extraction, matching and epipolar verification without the keypoints
    leaving HBM; the restatement runs on the fetched keypoints.  A pure shift
    is a degenerate epipolar scene (a family of F fits it), so this asserts
    agreement with the restatement and a sane inlier count, not a particular
    F."""
    import torch
    img = load_golden("bird_small")["image"]
    h, w = img.shape
    frames = np.stack([img, np.roll(img, 7, axis=1), np.roll(img, (5, -9), axis=(0, 1))])
    pairs = [(0, 1), (1, 2), (0, 2)]
    host = ctx.sift_batch(frames)
    t = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    c2 = pkg.Context(0, pkg.OpenCVProcessing)
    try:
        offs, _ = c2.sift_batch_device(t.data_ptr(), 3, w, h, t.stride(1), t.stride(0), fetch=False)
        before = c2.device_results()
        matches = c2.match_frames(offs, pairs)
        got = c2.verify_frames(offs, pairs, matches, model="fundamental")
        assert c2.device_results() == before  # only read
        for (a, b), mt, g in zip(pairs, matches, got):
            rec = E.records(host[a].keypoints_array, host[b].keypoints_array, mt)
            want = E.verify(rec, 3.0, 1024, 0, 2)
            near = E.near_threshold_any(rec, 3.0, 1024, 0, 2)
            print(f"pair {(a, b)}: {g[2]} of ref {want[2]}; near the threshold: {near}")
            assert near == []
            d = _assert_refit_equal(g, want, rec, (a, b))
            print(f"Sampson distances differ by {d:.3g} px")
            assert 200 <= g[2]["n_inliers"] <= g[2]["n_matches"] == len(rec)
    finally:
        c2.close()


@gpu
def test_sift_match_cli_verify_fundamental(pkg, ctx):
    """sift_match.py --verify 3 --model fundamental: the three lines of
    test_sift_match_cli, then the inlier count the restatement gives on the
    same matches."""
    import os
    import subprocess
    import sys
    from conftest import GOLDEN, ROOT
    paths = [os.path.join(GOLDEN, "jpeg", n + ".jpg") for n in ("bird_small", "tree_small")]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "sift-features_amd", "sift_match.py"), *paths,
                          "--processing", "opencv", "--ratio", "0.8", "--verify", "3", "--model", "fundamental"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    res = []
    for path in paths:
        with open(path, "rb") as f:
            res.append(ctx.sift_jpeg(f.read()))
    want = match_ref.match(res[1].descriptors, res[0].descriptors, 0.8, True)
    rec = E.records(res[1].keypoints_array, res[0].keypoints_array, want)
    info = E.verify(rec, 3.0, 1024, 0, 2)[2]
    near = E.near_threshold_any(rec, 3.0, 1024, 0, 2)
    print(out.stdout, info, near)
    assert near == []
    assert out.stdout.split("\n")[:4] == ["225 keypoints", "1270 keypoints", f"{len(want[0])} matches (ratio 0.8)",
                                          f"{info['n_inliers']} inliers (fundamental, threshold 3)"]
