"""Pins epipolar_ref.py, the numpy restatement of the epipolar verification
(RANSAC fundamental matrix; LABELLED EXTENSION) that test_gpu_verify_epipolar.py
holds the GPU path against: the sampling, the 8-point solve, the planted
fixtures, the Jacobi against np.linalg.eigh, the rank-2 contract, a named
fixture per wrong variant, the fixtures' clearance from the threshold and the
refit's independence of the summation order.  No GPU."""
import functools

import numpy as np
import pytest

import epipolar_ref as E


@functools.lru_cache(maxsize=None)
def _case(m, share, seed, rounds=2):
    rec, good = E.planted(m, share, seed)
    trace = []
    return rec, good, E.verify(rec, 2.0, 512, seed, rounds, trace=trace), trace


@pytest.mark.parametrize("m", [8, 9, 64, 1000])
def test_sampling_distinct_in_range(m):
    for seed in (0, 1, 0xFFFFFFFF):
        idx = E.samples(seed, np.arange(2000), m)
        assert idx.shape == (2000, 8) and idx.min() >= 0 and idx.max() < m
        assert (np.diff(np.sort(idx, 1), axis=1) > 0).all()
    assert not np.array_equal(E.samples(1, np.arange(64), m), E.samples(2, np.arange(64), m)) or m == 8
    if m <= 64:  # every index is drawn by every draw, the first and the last included
        for k in range(8):
            assert set(np.unique(E.samples(0, np.arange(4000), m)[:, k])) == set(range(m))


def test_eight_exact_correspondences():
    """Eight noise-free matches: the 8-point F explains held-out noise-free
    matches of the same scene.  The bound is on the f64 solve (_f64_model: the
    rule with its f32 casts removed); the stored f32 F is held to f32's reach."""
    rng = np.random.default_rng(0)
    q = rng.uniform([20, 20], [620, 460], (208, 2))
    rec64 = np.concatenate([q, E.two_view(q, rng.uniform(4.0, 12.0, 208))], 1)
    assert E.sampson(rec64, E.true_f()).max() < 1e-9
    d = E.sampson(rec64[8:], _f64_model(rec64[:8]))
    print("held-out Sampson distance under the f64 8-point F:", d.max())
    assert d.max() < 1e-6
    f, valid = E.models(rec64[:8].astype(np.float32), 0, np.arange(4))
    assert valid.all() and (np.abs(f).max(1) == 1.0).all()
    assert max(E.sampson(rec64[:8].astype(np.float32), g).max() for g in f) < 1e-3


def _f64_model(rec64):
    """The rule's elimination on f64 records (no f32 rounding of inputs or of F): E.models with the casts removed."""
    bx = E._box(rec64[:, 0], rec64[:, 1]) + E._box(rec64[:, 2], rec64[:, 3])
    a = np.stack(E._rows(*E._normalise(rec64, bx)), 1)
    perm = list(range(9))
    for k in range(8):
        j = int(np.argmax(np.abs(a[k:, k:])))
        r, c = k + j // (9 - k), k + j % (9 - k)
        a[[k, r]] = a[[r, k]]
        a[:, [k, c]] = a[:, [c, k]]
        perm[k], perm[c] = perm[c], perm[k]
        for r_ in range(k + 1, 8):
            a[r_, k + 1:] = a[r_, k + 1:] - (a[r_, k] / a[k, k]) * a[k, k + 1:]
    g = [0.0] * 8 + [1.0]
    for k in range(7, -1, -1):
        s = -a[k, 8]
        for c in range(k + 1, 8):
            s = s - a[k, c] * g[c]
        g[k] = s / a[k, k]
    fp = np.zeros(9)
    fp[perm] = g
    F = E._denorm(fp.reshape(3, 3).tolist(), bx)
    return np.array(F)


@pytest.mark.parametrize("m,share,seed", E.REFIT_CASES)
def test_planted_fixtures_recover(m, share, seed):
    rec, good, (F, mask, info), _ = _case(m, share, seed)
    print(m, share, info, "planted", good.sum(), "kept", (mask & good).sum())
    assert info["best_hypothesis"] >= 0 and info["refits"] >= 1
    assert (mask & good).sum() >= 0.95 * good.sum()
    assert info["n_inliers"] == mask.sum()
    assert np.abs(F).max() == 1.0


@pytest.mark.parametrize("m,share,seed", E.REFIT_CASES)
def test_jacobi_matches_eigh(m, share, seed):
    """The smallest eigenvector of the fixtures' moment matrices against LAPACK: this fixes SWEEPS."""
    rec, _, (_, mask, _), _ = _case(m, share, seed)
    M = E.moments(rec, mask)
    w, v = np.linalg.eigh(np.array(M))
    f = np.array(E._smallest([list(r) for r in M]))
    f *= np.sign(f @ v[:, 0])
    assert np.abs(f - v[:, 0]).max() <= 1e-10
    w2, _ = E._jacobi([list(r) for r in M])
    assert np.allclose(sorted(w2), w, rtol=0, atol=1e-12 * w[-1])


def test_jacobi_ties_and_zero_rotations():
    assert E._smallest([[2.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) == [0.0, 1.0, 0.0]  # lowest index on ties
    v = E._smallest([[2.0, 1.0], [1.0, 2.0]])
    assert abs(abs(v[0]) - 2 ** -0.5) < 1e-15 and v[0] == -v[1]


@pytest.mark.parametrize("m,share,seed", E.REFIT_CASES)
def test_rank_two_iff_refit(m, share, seed):
    rec, _, (F, _, info), _ = _case(m, share, seed)
    assert info["refits"] >= 1
    s = np.linalg.svd(F.astype(np.float64), compute_uv=False)
    assert s[2] / s[0] < 1e-6
    F0, _, info0 = E.verify(rec, 2.0, 512, seed, 0)
    s0 = np.linalg.svd(F0.astype(np.float64), compute_uv=False)
    assert info0["refits"] == 0 and info0["best_hypothesis"] == info["best_hypothesis"]
    print("sigma3 / sigma1 raw", s0[2] / s0[0], "refit", s[2] / s[0])


def test_no_model():
    for m in range(8):
        F, mask, info = E.verify(E.planted(m, 1.0, 1)[0], 2.0, 64, 0, 2)
        assert not F.any() and not mask.any() and len(mask) == m
        assert info == dict(n_matches=m, n_inliers=0, best_hypothesis=-1, refits=0)
    import verify_ref
    rec = verify_ref.duplicates()
    f, valid = E.models(rec, 0, np.arange(64))
    assert not valid.any() and not f.any()  # repeated rows: an exact zero pivot
    for rounds in (0, 2):
        assert E.verify(rec, 2.0, 64, 0, rounds)[2] == dict(n_matches=30, n_inliers=0, best_hypothesis=-1, refits=0)


# ---- a named fixture per wrong variant ----------------------------------------
def test_variant_tie_high_and_repeat():
    rec = E.eight_exact()
    assert (np.sort(E.samples(0, np.arange(64), 8), 1) == np.arange(8)).all()  # every hypothesis: the same eight
    F, mask, info = E.verify(rec, 2.0, 64, 0, 0)
    assert info["best_hypothesis"] == 0 and info["n_inliers"] == 8 and mask.all()
    assert E.verify(rec, 2.0, 64, 0, 0, variant="tie_high")[2]["best_hypothesis"] == 63
    # with replacement eight draws of eight repeat a match: equal rows, an exact zero pivot, no model
    assert (np.diff(np.sort(E.samples(0, np.arange(64), 8, "repeat"), 1), axis=1) == 0).any(1).all()
    assert E.verify(rec, 2.0, 64, 0, 0, variant="repeat")[2]["best_hypothesis"] == -1


def test_variant_thr_lt_and_one_sided():
    rec = E.threshold_exact()
    assert E.box(rec) == (128.0, 96.0, 2.0 ** -7, 128.0, 128.0, 2.0 ** -7)
    F, mask, info = E.verify(rec, 3.0, 64, 0, 0)
    assert np.array_equal(F, np.array([[0, 0, 0], [0, 0, -0.75], [0, 1, 0]], np.float32))  # residue below f32's reach
    assert mask.all() and info["n_inliers"] == 40
    x, y, X, Y = rec[0]
    e, d = np.float32(Y) * np.float32(-0.75) + np.float32(y), np.float32(0.75 * 0.75 + 1.0)
    assert e * e == np.float32(9.0) * d  # exactly on the threshold
    F2, mask2, info2 = E.verify(rec, 3.0, 64, 0, 0, variant="thr_lt")
    assert not mask2[0] and mask2[1:].all() and info2["n_inliers"] == 39
    # without the train-side gradient d = .75^2, and match 0 is 5 px away instead of 3
    F3, mask3, info3 = E.verify(rec, 3.0, 64, 0, 0, variant="one_sided")
    assert not mask3[0] and mask3[1:].all() and info3["n_inliers"] == 39


def test_variant_no_colpivot():
    rec = E.sideways()
    F, mask, info = E.verify(rec, 2.0, 64, 0, 0)
    assert info == dict(n_matches=40, n_inliers=40, best_hypothesis=0, refits=0)
    assert F[2, 2] == 0 and np.array_equal(np.abs(F), np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0]], np.float32))
    assert F[1, 2] == -F[2, 1]
    # rows only, f'[8] = 1: hypothesis 0 meets an exact zero pivot
    f, valid = E.models(rec, 0, np.arange(1), variant="no_colpivot")
    assert not valid[0]
    assert E.verify(rec, 2.0, 64, 0, 0, variant="no_colpivot")[2]["best_hypothesis"] != 0


# ---- clearance from the threshold ------------------------------------------------
@pytest.mark.parametrize("m,share,seed", E.REFIT_CASES)
def test_refit_fixtures_stay_clear_of_the_threshold(m, share, seed):
    rec = E.planted(m, share, seed)[0]
    for rounds in (1, 2):
        assert E.near_threshold_any(rec, 2.0, 512, seed, rounds) == []


def test_segment_fixtures_stay_clear_of_the_threshold():
    kps, offs, pairs, matches, recs = E.segments()
    assert len(pairs) == len(E.SEG_MATCHES) + 1 and [len(r) for r in recs[:-1]] == E.SEG_MATCHES
    for (a, b), mt, rec in zip(pairs, matches, recs):
        assert np.array_equal(E.records(kps[offs[a]:offs[a + 1]], kps[offs[b]:offs[b + 1]], mt), rec)
        for rounds in (0, 1, 2):
            assert E.near_threshold_any(rec, 2.0, 300, 5, rounds) == []


# ---- summation order ----------------------------------------------------------------
@pytest.mark.parametrize("m,share,seed", E.REFIT_CASES)
def test_refit_summation_order(m, share, seed):
    rec, _, (_, mask, _), trace = _case(m, share, seed)
    rng = np.random.default_rng(seed)
    base, base64 = E.refit(rec, mask), E.refit(rec, mask, f64=True)
    worst = 0.0
    for _ in range(3):
        order = rng.permutation(int(mask.sum()))
        assert np.array_equal(E.refit(rec, mask, order).view(np.uint32), base.view(np.uint32))
        worst = max(worst, np.abs(E.refit(rec, mask, order, f64=True) - base64).max())
    print("f64 F moves by", worst)
    assert worst <= 1e-10
    assert len(E.SUMS) == 45 and len(set(E.SUMS)) == 45
