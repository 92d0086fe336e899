"""The two geometric verifications with progressive (PROSAC) sampling on the GPU
(sift_mi_verify_matches_progressive, sift_mi_verify_pairs_progressive_device
and their epipolar forms; the ranking gather and the progressive models
kernels of csrc/verify.hip and csrc/verify_epipolar.hip) against their numpy
restatement (prosac_ref.py, pinned by test_prosac_ref_cpu.py).  LABELLED
EXTENSION: the crate has nothing like it.

Without refits everything is bit-exact: the model as bit patterns, the mask in
the caller's match order, n_inliers, best_hypothesis.  With refits the
siblings' contract holds (test_gpu_verify.py, test_gpu_verify_epipolar.py):
masks, counts and accepted rounds equal, the models within 1e-3 px on the
pair's query points (homography) or 1e-3 px of Sampson distance on its matches
(fundamental matrix); the refit fixtures keep every match 1e-2 px from the
threshold (test_prosac_ref_cpu.py), so that bound implies equal masks."""
import ctypes
import functools

import numpy as np
import pytest
from conftest import load_golden

import epipolar_ref as E
import prosac_ref as P
import verify_ref as V

gpu = pytest.mark.gpu

MODELS = ("homography", "fundamental")
K = {"homography": 4, "fundamental": 8}
ROWS, STAGE = 512, 1024  # csrc/sift_kernels.h kVerifyRankRows, kVerifyRankStage (= kVerifyChunk)


def _arrays(rec):
    """A record list as two keypoint arrays and the identity matches."""
    rec = np.asarray(rec, np.float32).reshape(-1, 4)
    m = len(rec)
    kq, kt = np.zeros((m, 5), np.float32), np.zeros((m, 5), np.float32)
    kq[:, :2], kt[:, :2] = rec[:, :2], rec[:, 2:]
    i = np.arange(m, dtype=np.int32)
    return kq, kt, (i, i, np.zeros(m, np.float32))


def _gpu(ctx, rec, q, model, thr, it, seed, rounds):
    return ctx.verify_matches(*_arrays(rec), threshold=thr, iterations=it, seed=seed, refit_rounds=rounds,
                              model=model, sampling="progressive", quality=q)


def _assert_bit_exact(got, want, what=None):
    (H, mask, info), (rH, rmask, rinfo) = got, want
    assert info == rinfo, (what, info, rinfo)
    assert H.dtype == np.float32 and H.shape == (3, 3) and mask.dtype == bool
    assert np.array_equal(H.view(np.uint32), rH.view(np.uint32)), (what, H, rH)
    assert np.array_equal(mask, rmask), what
    assert info["n_inliers"] == mask.sum() <= info["n_matches"] == len(mask)


def _model_distance(model, rec, a, b):
    """How far two models are apart on the pair, in px (the siblings' measures)."""
    if model == "homography":
        return np.abs(V.project(a, rec[:, :2]) - V.project(b, rec[:, :2])).max()
    d = np.abs(E.sampson(rec, a) - E.sampson(rec, b))
    return d[np.isfinite(d)].max()


@functools.lru_cache(maxsize=None)
def _planted(model, m, seed, share=0.6):
    rec, good = P.MODELS[model][0].planted(m, share, seed)
    q = P.synthetic_quality(good, seed)
    rec.setflags(write=False)
    q.setflags(write=False)
    return rec, q


@functools.lru_cache(maxsize=None)
def _ref(model, m, seed, it, rounds=0):
    rec, q = _planted(model, m, seed)
    return P.verify(rec, q, model, 2.0, it, seed, rounds)


# ---- bit-exact without refits ---------------------------------------------------
@gpu
@pytest.mark.parametrize("m", ["0", "k-1", "k", "k+1", 63, 64, 65, ROWS - 1, ROWS, ROWS + 1, STAGE - 1, STAGE,
                               STAGE + 1, 2000])
@pytest.mark.parametrize("model", MODELS)
def test_bit_exact_match_counts(ctx, model, m):
    """The wave size, the ranking gather's rows per workgroup, its stage (the
    record chunk as well) and several of each; 300 hypotheses: two workgroups
    per pair, the second partly filled."""
    m = eval(m, {"k": K[model]}) if isinstance(m, str) else m
    rec, q = _planted(model, m, 100 + m)
    got = _gpu(ctx, rec, q, model, 2.0, 300, 100 + m, 0)
    _assert_bit_exact(got, _ref(model, m, 100 + m, 300), m)
    if m >= 63:
        assert got[2]["n_inliers"] > 0.5 * m  # the planted 60 %


@gpu
@pytest.mark.parametrize("it", [1, 255, 256, 257, 1024])
@pytest.mark.parametrize("model", MODELS)
def test_bit_exact_iterations(ctx, model, it):
    rec, q = _planted(model, 300, 9)
    _assert_bit_exact(_gpu(ctx, rec, q, model, 2.0, it, 9, 0), _ref(model, 300, 9, it), it)


@gpu
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("model", MODELS)
def test_uniform_tail(ctx, model, extra):
    """N = k and N = k + 1 at 1024 hypotheses: past T'_N the sample is the uniform one."""
    k = K[model]
    n = P.subset_size(np.arange(1024), k + extra, k, 1024)
    assert (n == k + extra + 1).sum() > 100  # the tail is most of the call (N = k) or a tenth of it
    rec, _ = P.MODELS[model][0].planted(k + extra, 1.0, 40 + extra)
    q = np.arange(k + extra, 0, -1).astype(np.float32)
    _assert_bit_exact(_gpu(ctx, rec, q, model, 2.0, 1024, 3, 0), P.verify(rec, q, model, 2.0, 1024, 3, 0))


@gpu
def test_variant_fixtures(ctx):
    """The fixtures on which test_prosac_ref_cpu.py tells the wrong variants
    from the rule: the GPU gives the rule's answer, none of theirs."""
    seen = set()
    for variant in P.VARIANTS:
        rec, q, model, thr, it, seed = P.variant_fixture(variant)
        right = P.verify(rec, q, model, thr, it, seed, 0)
        if (len(rec), it) not in seen:
            seen.add((len(rec), it))
            _assert_bit_exact(_gpu(ctx, rec, q, model, thr, it, seed, 0), right, variant)
        wrong = P.verify(rec, q, model, thr, it, seed, 0, variant=variant)
        assert not (right[2] == wrong[2] and np.array_equal(right[1], wrong[1])
                    and np.array_equal(right[0].view(np.uint32), wrong[0].view(np.uint32))), variant
    assert len(seen) == 4  # the value fixture, tied_triples, boundary_twelve, tail_six


# ---- quality shapes --------------------------------------------------------------
@gpu
@pytest.mark.parametrize("model", MODELS)
def test_quality_shapes(ctx, model):
    k = K[model]
    rec, _ = _planted(model, 300, 9)
    m = len(rec)
    # all equal: rank = identity, whatever the value
    for value in (0.0, 7.0, 3.0e38):
        q = np.full(m, value, np.float32)
        assert P.rank_order(q).tolist() == list(range(m))
        _assert_bit_exact(_gpu(ctx, rec, q, model, 2.0, 300, 1, 0), P.verify(rec, q, model, 2.0, 300, 1, 0), value)
    # strictly descending: the full reversal
    q = np.arange(m, 0, -1).astype(np.float32)
    assert P.rank_order(q).tolist() == list(range(m))[::-1]
    _assert_bit_exact(_gpu(ctx, rec, q, model, 2.0, 300, 1, 0), P.verify(rec, q, model, 2.0, 300, 1, 0), "reversed")
    # integer-valued with ties across every n_h boundary of the first 64 hypotheses: one tied
    # group covers ranks 0 .. n_63 + 1 (in a shuffled caller order, so the index decides), pairs after it
    n63 = int(P.subset_size([63], m, k, 300)[0])
    assert k < n63 < m - 10
    ranked = np.concatenate([np.full(n63 + 2, 5.0), 6.0 + (np.arange(m - n63 - 2) // 2)]).astype(np.float32)
    q = ranked[np.random.default_rng(2).permutation(m)]
    order = P.rank_order(q)
    for n in range(k, n63 + 1):  # the boundary between the best n and the rest runs through equal qualities
        assert q[order[n - 1]] == q[order[n]]
    _assert_bit_exact(_gpu(ctx, rec, q, model, 2.0, 300, 1, 0), P.verify(rec, q, model, 2.0, 300, 1, 0), "ties")
    wrong = P.verify(rec, q, model, 2.0, 300, 1, 0, variant="tie_high")
    assert wrong[2] != P.verify(rec, q, model, 2.0, 300, 1, 0)[2]


@gpu
@pytest.mark.parametrize("model", MODELS)
def test_quality_null_uses_the_matches_distance(ctx, model):
    rec, q = _planted(model, 300, 9)
    kq, kt, (qi, ti, _) = _arrays(rec)
    got = ctx.verify_matches(kq, kt, (qi, ti, np.asarray(q)), threshold=2.0, iterations=300, seed=1, refit_rounds=0,
                             model=model, sampling="progressive")
    _assert_bit_exact(got, P.verify(rec, q, model, 2.0, 300, 1, 0))
    # an explicit quality wins over the distances
    got = ctx.verify_matches(kq, kt, (qi, ti, np.asarray(q)[::-1].copy()), threshold=2.0, iterations=300, seed=1,
                             refit_rounds=0, model=model, sampling="progressive", quality=q)
    _assert_bit_exact(got, P.verify(rec, q, model, 2.0, 300, 1, 0))


# ---- the caller's order -------------------------------------------------------------
@gpu
@pytest.mark.parametrize("model", MODELS)
def test_permuting_the_matches_permutes_the_mask(ctx, model):
    rec, _ = P.MODELS[model][0].planted(700, 0.5, 3)
    rng = np.random.default_rng(1)
    q = rng.permutation(700).astype(np.float32) + 1  # no ties
    g, mask, info = _gpu(ctx, rec, q, model, 2.0, 256, 3, 0)
    assert info["n_inliers"] >= 200
    perm = rng.permutation(700)
    g2, mask2, info2 = _gpu(ctx, rec[perm], q[perm], model, 2.0, 256, 3, 0)
    assert info2 == info and np.array_equal(g2.view(np.uint32), g.view(np.uint32))
    assert np.array_equal(mask2, mask[perm])
    _assert_bit_exact((g, mask, info), P.verify(rec, q, model, 2.0, 256, 3, 0))


# ---- segments ---------------------------------------------------------------------
def _segment_quality(matches, seed=4):
    """Per pair integer qualities in 1..500 with 0 at both ends of the pair's
    slice: in the call's quality array every pair's neighbours hold 0, so a
    key read past a pair's bound would rank first and change the samples."""
    rng = np.random.default_rng(seed)
    out = []
    for mt in matches[:-1]:
        q = rng.integers(1, 501, len(mt[0])).astype(np.float32)
        q[:1] = 0
        q[-1:] = 0
        out.append(q)
    return out


@pytest.fixture(scope="module", params=MODELS)
def arena(request):
    import torch
    mod = P.MODELS[request.param][0]
    kps, offs, pairs, matches, recs = mod.segments()
    quality = _segment_quality(matches)
    quality.append(quality[mod.SEG_TWICE])
    t = torch.from_numpy(kps.copy()).cuda()
    torch.cuda.synchronize()
    return request.param, t, kps, offs, pairs, matches, recs, quality


@gpu
@pytest.mark.parametrize("rounds", [0, 2])
def test_segment_pairs(ctx, arena, rounds):
    model, t, kps, offs, pairs, matches, recs, quality = arena
    mod = P.MODELS[model][0]
    assert len(pairs) == 10
    got = ctx.verify_pairs_device(t.data_ptr(), offs, pairs, matches, threshold=2.0, iterations=300, seed=5,
                                  refit_rounds=rounds, model=model, sampling="progressive", quality=quality)
    assert len(got) == len(pairs)
    for p, ((a, b), mt, rec, q, g) in enumerate(zip(pairs, matches, recs, quality, got)):
        assert g[2]["n_inliers"] <= g[2]["n_matches"] == len(rec)
        own = ctx.verify_matches(kps[offs[a]:offs[a + 1]], kps[offs[b]:offs[b + 1]], mt, threshold=2.0,
                                 iterations=300, seed=5, refit_rounds=rounds, model=model, sampling="progressive",
                                 quality=q)
        _assert_bit_exact(g, own, p)  # a pair's place in the call is not an input
        want = P.verify(rec, q, model, 2.0, 300, 5, rounds)
        if rounds == 0:
            _assert_bit_exact(g, want, p)
        else:
            assert P.near_threshold_any(rec, q, model, 2.0, 300, 5, rounds) == []
            assert g[2] == want[2] and np.array_equal(g[1], want[1]), (p, g[2], want[2])
            if want[2]["best_hypothesis"] >= 0:
                assert _model_distance(model, rec, g[0], want[0]) <= 1e-3
    _assert_bit_exact(got[mod.SEG_TWICE], got[-1])  # the pair listed twice
    for p, m in enumerate(mod.SEG_MATCHES):
        if m >= 64:
            assert got[p][2]["n_inliers"] > 0.5 * m


# ---- what it is for -----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", P.VALUE_CASES)
def test_progressive_recovers_what_uniform_misses(ctx, case):
    """The value fixtures exactly as test_prosac_ref_cpu.py has them: 400
    matches at planted shares 0.25 / 0.15, threshold 2.0, 1024 hypotheses, no
    refit.  Uniform sampling recovers at most half of the planted inliers,
    progressive sampling at least 95 %."""
    model, m, share, seed = case
    rec, good, q = P.value_fixture(*case)
    uni = ctx.verify_matches(*_arrays(rec), threshold=2.0, iterations=1024, seed=seed, refit_rounds=0, model=model)
    pro = _gpu(ctx, rec, q, model, 2.0, 1024, seed, 0)
    _assert_bit_exact(uni, P.MODELS[model][0].verify(rec, 2.0, 1024, seed, 0))
    _assert_bit_exact(pro, P.verify(rec, q, model, 2.0, 1024, seed, 0))
    n, got_u, got_p = int(good.sum()), int((uni[1] & good).sum()), int((pro[1] & good).sum())
    print(f"{case}: planted {n}, uniform recovers {got_u}, progressive {got_p}")
    assert got_u <= 0.5 * n
    assert got_p >= 0.95 * n


# ---- refit ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("rounds", [1, 2])
@pytest.mark.parametrize("case", P.REFIT_CASES)
def test_refit(ctx, case, rounds):
    model, m, share, seed = case
    rec, good, q = P.value_fixture(*case)
    rG, rmask, rinfo = P.verify(rec, q, model, 2.0, 512, seed, rounds)
    G, mask, info = _gpu(ctx, rec, q, model, 2.0, 512, seed, rounds)
    d = _model_distance(model, rec, G, rG)
    print(f"{case} rounds {rounds}: refits {info['refits']} inliers {info['n_inliers']} (ref {rinfo['n_inliers']}), "
          f"models differ by {d:.3g} px")
    assert info == rinfo
    assert np.array_equal(mask, rmask)
    assert d <= 1e-3
    assert info["refits"] >= 1 and (mask & good).sum() >= 0.95 * good.sum()


# ---- the old call through the new keyword ---------------------------------------------------
@gpu
@pytest.mark.parametrize("model", MODELS)
def test_sampling_uniform_is_the_old_call(ctx, model):
    rec, _ = _planted(model, 300, 9)
    for rounds in (0, 2):
        old = ctx.verify_matches(*_arrays(rec), threshold=2.0, iterations=300, seed=9, refit_rounds=rounds, model=model)
        new = ctx.verify_matches(*_arrays(rec), threshold=2.0, iterations=300, seed=9, refit_rounds=rounds, model=model,
                                 sampling="uniform")
        _assert_bit_exact(new, old, rounds)
    _assert_bit_exact(ctx.verify_matches(*_arrays(rec), 2.0, 300, 9, 0, model, "uniform"),
                      P.MODELS[model][0].verify(rec, 2.0, 300, 9, 0))
    with pytest.raises(ValueError):
        ctx.verify_matches(*_arrays(rec), sampling="uniform", quality=np.ones(300, np.float32))
    with pytest.raises(ValueError):
        ctx.verify_matches(*_arrays(rec), sampling="prosac")
    with pytest.raises(ValueError):
        ctx.verify_matches(*_arrays(rec), sampling="progressive", quality=np.ones(299, np.float32))


# ---- EINVAL ------------------------------------------------------------------------------
def _raw(pkg, ctx, model, d_ptr, offs, pairs, matches, po, quality, prm, models=True, mask=True):
    from sift_features_amd import _lib
    L = pkg.lib()
    c_offs = None if offs is None else (ctypes.c_size_t * len(offs))(*[int(v) for v in offs])
    c_pairs = None if pairs is None else (_lib.SegPair * max(1, len(pairs)))(*[_lib.SegPair(a, b) for a, b in pairs])
    c_m = None if matches is None else (_lib.Match * max(1, len(matches)))(*[_lib.Match(*m) for m in matches])
    c_po = None if po is None else (ctypes.c_size_t * len(po))(*po)
    c_q = None if quality is None else (ctypes.c_float * max(1, len(quality)))(*quality)
    c_prm = None if prm is None else ctypes.byref(_lib.RansacParams(*prm))
    n_pairs = 0 if pairs is None else len(pairs)
    out = (_lib.Homography * max(1, n_pairs))() if models else None
    msk = (ctypes.c_uint8 * 64)() if mask else None
    call = (L.sift_mi_verify_pairs_progressive_device if model == "homography"
            else L.sift_mi_verify_pairs_epipolar_progressive_device)
    return call(ctx._h, ctypes.c_void_p(d_ptr), c_offs, 0 if offs is None else len(offs) - 1, c_pairs, n_pairs, c_m,
                c_po, c_q, c_prm, out, msk)


@gpu
@pytest.mark.parametrize("model", MODELS)
def test_progressive_einval(pkg, ctx, model):
    import torch
    rec, _ = _planted(model, 12, 1)
    kq, kt, _m = _arrays(rec)
    t = torch.from_numpy(np.concatenate([kq, kt])).cuda()
    torch.cuda.synchronize()
    d, offs, pairs, po, prm = t.data_ptr(), [0, 12, 24], [(0, 1)], [0, 12], (2.0, 64, 0, 1)
    mt = [(i, i, float(i)) for i in range(12)]
    q = [float(12 - i) for i in range(12)]
    run = lambda *a, **kw: _raw(pkg, ctx, model, *a, **kw)
    assert run(d, offs, pairs, mt, po, q, prm) == 0
    assert run(d, offs, pairs, mt, po, None, prm) == 0  # quality may be null
    nan, inf = float("nan"), float("inf")
    # a quality that is NaN, infinite or has its sign bit set (-0.0 included), anywhere in the array
    for bad in (nan, -nan, inf, -inf, -1.0, -0.0, -1e-45):
        for at in (0, 5, 11):
            assert run(d, offs, pairs, mt, po, q[:at] + [bad] + q[at + 1:], prm) == -1, (bad, at)
            assert b"quality" in pkg.lib().sift_mi_last_error()
        # the same in the matches' distance when quality is null, and only then
        bad_mt = mt[:5] + [(5, 5, bad)] + mt[6:]
        assert run(d, offs, pairs, bad_mt, po, None, prm) == -1, bad
        assert b"distance" in pkg.lib().sift_mi_last_error()
        assert run(d, offs, pairs, bad_mt, po, q, prm) == 0, bad
        with pytest.raises(pkg.SiftMiError):
            ctx.verify_matches(kq, kt, (np.arange(12), np.arange(12)), model=model, sampling="progressive",
                               quality=np.array(q[:3] + [bad] + q[4:], np.float32))
    assert run(d, offs, pairs, mt, po, [0.0, 3.4e38, 1e-45] + q[3:], prm) == 0  # +0, the largest, a denormal
    # a quality outside the call's matches is not read
    assert _raw(pkg, ctx, model, d, offs, pairs, [(0, 0, nan)] + mt, [1, 13], [nan] + q, prm) == 0
    # the siblings' own checks
    assert run(None, offs, pairs, mt, po, q, prm) == -1
    assert run(d, None, pairs, mt, po, q, prm) == -1
    assert run(d, offs, None, mt, po, q, prm) == -1
    assert run(d, offs, pairs, None, po, q, prm) == -1
    assert run(d, offs, pairs, mt, None, q, prm) == -1
    assert run(d, offs, pairs, mt, po, q, None) == -1
    assert run(d, offs, pairs, mt, po, q, prm, models=False) == -1
    assert run(d, offs, pairs, mt, po, q, prm, mask=False) == -1
    for thr in (nan, inf, 0.0, -1.0):
        assert run(d, offs, pairs, mt, po, q, (thr, 64, 0, 1)) == -1, thr
    assert run(d, offs, pairs, mt, po, q, (2.0, 0, 0, 1)) == -1
    assert run(d, offs, pairs, mt, po, q, (2.0, 65537, 0, 1)) == -1
    assert run(d, offs, pairs, mt, po, q, (2.0, 64, 0, 9)) == -1
    assert run(d, offs, pairs, mt, po, q, (2.0, 64, 0, 8)) == 0
    assert run(d, offs, [(0, 2)], mt, po, q, prm) == -1
    assert run(d, offs, [(2, 1)], mt, po, q, prm) == -1
    assert run(d, [0, 14, 12], pairs, mt, po, q, prm) == -1
    assert run(d, offs, [(0, 1), (0, 1)], mt, [0, 12, 4], q, prm) == -1
    for bad in ((12, 0), (0, 12), (-1, 0), (0, -1)):
        assert run(d, offs, pairs, mt[:11] + [(*bad, 1.0)], po, q, prm) == -1, bad
    assert b"segment" in pkg.lib().sift_mi_last_error()
    # still usable afterwards, and no pairs at all is an empty result
    assert run(d, offs, pairs, mt, po, q, prm) == 0
    assert run(d, offs, [], mt, [0], q, prm) == 0
    qa = np.array(q, np.float32)
    _assert_bit_exact(_gpu(ctx, rec, qa, model, 2.0, 64, 0, 0), P.verify(rec, qa, model, 2.0, 64, 0, 0))


# ---- end to end -----------------------------------------------------------------------------
@gpu
def test_verify_frames_progressive_end_to_end(pkg, ctx):
    """The three frames of test_verify_frames_end_to_end: extraction, matching
    and progressive verification (ranked by the matcher's distances) without
    the keypoints leaving HBM; the restatement runs on the fetched keypoints."""
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
        got = c2.verify_frames(offs, pairs, matches, sampling="progressive")
        assert c2.device_results() == before  # only read
        pts = np.array([[w / 2, h / 2], [0, 0], [w - 1, h - 1]], np.float64)
        for (a, b), mt, (H, mask, info) in zip(pairs, matches, got):
            rec = V.records(host[a].keypoints_array, host[b].keypoints_array, mt)
            rH, rmask, rinfo = P.verify(rec, mt[2], "homography", 3.0, 1024, 0, 2)
            dev = np.abs(V.project(H, pts) - (pts + shifts[a, b])).max()
            d = np.abs(V.project(H, rec[:, :2]) - V.project(rH, rec[:, :2])).max()
            print(f"pair {(a, b)}: {info} of ref {rinfo}; corners off the shift by {dev:.3g} px; "
                  f"projections differ by {d:.3g} px")
            assert P.near_threshold_any(rec, mt[2], "homography", 3.0, 1024, 0, 2) == []
            assert info == rinfo and np.array_equal(mask, rmask) and d <= 1e-3
            assert info["n_inliers"] >= 200
            assert dev <= 0.25
    finally:
        c2.close()


@gpu
def test_sift_match_cli_progressive(pkg, ctx):
    """sift_match.py --verify 3 --progressive: the three lines of
    test_sift_match_cli, then the inlier count the restatement gives on the
    same matches ranked by their distance."""
    import os
    import subprocess
    import sys
    from conftest import GOLDEN, ROOT
    paths = [os.path.join(GOLDEN, "jpeg", n + ".jpg") for n in ("bird_small", "tree_small")]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "sift-features_amd", "sift_match.py"), *paths,
                          "--processing", "opencv", "--ratio", "0.8", "--verify", "3", "--progressive"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    res = []
    for path in paths:
        with open(path, "rb") as f:
            res.append(ctx.sift_jpeg(f.read()))
    want = ctx.match_descriptors(res[1].descriptors, res[0].descriptors, cross_check=True, ratio=0.8)
    rec = V.records(res[1].keypoints_array, res[0].keypoints_array, want)
    info = P.verify(rec, want[2], "homography", 3.0, 1024, 0, 2)[2]
    near = P.near_threshold_any(rec, want[2], "homography", 3.0, 1024, 0, 2)
    print(out.stdout, info, near)
    assert near == []
    assert out.stdout.split("\n")[:4] == ["225 keypoints", "1270 keypoints", f"{len(want[0])} matches (ratio 0.8)",
                                          f"{info['n_inliers']} inliers (homography, threshold 3, progressive)"]
