"""Pins the numpy restatement of the geometric verification (verify_ref.py)
without a GPU: the sampling, the minimal solve, the planted fixtures, one named
fixture per deliberately wrong variant, and the distance of the refit
fixtures' matches from the threshold (what lets test_gpu_verify.py demand
equal masks after a refit)."""
import ctypes

import numpy as np
import pytest

import verify_ref as V


# ---- sampling -------------------------------------------------------------------
@pytest.mark.parametrize("m", [4, 5, 7, 1000])
def test_samples_distinct_in_range(m):
    s = V.samples(12345, np.arange(4096), m)
    assert s.shape == (4096, 4) and s.min() >= 0 and s.max() < m
    assert all(len(set(r)) == 4 for r in s.tolist())
    if m == 4:
        assert all(sorted(r) == [0, 1, 2, 3] for r in s.tolist())


def test_samples_uniform():
    """m = 5, 4096 hypotheses of 4 draws: each index expects 16384 / 5 = 3277
    picks, standard deviation sqrt(16384 * 0.2 * 0.8) = 51; five sigma."""
    cnt = np.bincount(V.samples(0, np.arange(4096), 5).ravel(), minlength=5)
    assert cnt.sum() == 16384 and np.all(np.abs(cnt - 16384 / 5) < 5 * 51.2), cnt


def test_samples_do_not_depend_on_anything_else():
    a = V.samples(7, np.arange(100, 200), 50)
    assert np.array_equal(a, V.samples(7, np.arange(0, 200), 50)[100:])
    assert not np.array_equal(a, V.samples(8, np.arange(100, 200), 50))
    assert any(len(set(r)) < 4 for r in V.samples(7, np.arange(256), 5, variant="repeat").tolist())


def test_mix32_known_values():
    # the lowbias32 finaliser: 0 is its fixed point, and it is a bijection on a sample
    assert int(V.mix32(0)) == 0
    v = V.mix32(np.arange(1, 1 << 16))
    assert len(np.unique(v)) == len(v) and v.max() <= 0xFFFFFFFF


# ---- model -----------------------------------------------------------------------
def test_four_exact_correspondences_give_h_back():
    rec = V.four()
    h, valid = V.models(rec, 0, np.arange(8))
    assert valid.all()
    for g in h:
        assert np.abs(g.reshape(3, 3) - V.H_MILD).max() < 1e-4 * np.abs(V.H_MILD).max()
        assert np.hypot(*(V.project(g.reshape(3, 3), rec[:, :2]) - rec[:, 2:]).T).max() < 1e-3
    H, mask, info = V.verify(rec, 2.0, 64, 0, 0)
    assert mask.all() and info == dict(n_matches=4, n_inliers=4, best_hypothesis=0, refits=0)


@pytest.mark.parametrize("m", [0, 1, 3])
def test_fewer_than_four_matches(m):
    H, mask, info = V.verify(V.planted(8, 1.0, 1)[0][:m], 2.0, 64, 0, 2)
    assert not H.any() and mask.shape == (m,) and not mask.any()
    assert info == dict(n_matches=m, n_inliers=0, best_hypothesis=-1, refits=0)


@pytest.mark.parametrize("rec", [V.collinear(), V.duplicates()], ids=["collinear", "duplicates"])
def test_degenerate_sets_have_no_model(rec):
    H, mask, info = V.verify(rec, 2.0, 256, 0, 2)
    assert not H.any() and not mask.any() and info["best_hypothesis"] == -1 and info["n_inliers"] == 0


# ---- planted fixtures ---------------------------------------------------------------
@pytest.mark.parametrize("m,share,seed", V.REFIT_CASES)
def test_planted_recovered(m, share, seed):
    """At least 95 % of the planted inliers, at most 1 % of the mask false
    (the noise is +-0.5 px per axis, at most 0.71 px, under the threshold 2)."""
    rec, good = V.planted(m, share, seed)
    H, mask, info = V.verify(rec, 2.0, 512, seed, 2)
    assert (mask & good).sum() >= 0.95 * good.sum(), ((mask & good).sum(), good.sum())
    assert (mask & ~good).sum() <= 0.01 * mask.sum(), ((mask & ~good).sum(), mask.sum())
    assert info["refits"] >= 1 and info["n_inliers"] == mask.sum()
    assert info["n_inliers"] >= V.verify(rec, 2.0, 512, seed, 0)[2]["n_inliers"]


def _clear_of_threshold(rec, thr, it, seed, rounds):
    assert V.near_threshold_any(rec, thr, it, seed, rounds) == []
    H, mask, info = V.verify(rec, thr, it, seed, rounds)
    if info["best_hypothesis"] >= 0:
        assert np.array_equal(mask, V.residuals(rec, H) <= thr)


@pytest.mark.parametrize("rounds", [1, 2])
@pytest.mark.parametrize("m,share,seed", V.REFIT_CASES)
def test_refit_fixtures_stay_clear_of_the_threshold(m, share, seed, rounds):
    """No match within 1e-2 px of the threshold under any H a refit round
    scores (so every accept / reject decision has that margin) nor under the
    final one: the GPU's H differs from the restatement's by f32 rounding of
    sums taken in another order (1e-3 px at most, test_gpu_verify.py), so the
    masks, counts and accepted rounds must be equal."""
    _clear_of_threshold(V.planted(m, share, seed)[0], 2.0, 512, seed, rounds)


@pytest.mark.parametrize("rounds", [1, 2])
def test_segment_fixtures_stay_clear_of_the_threshold(rounds):
    """The same for the pairs of segments() as test_segment_pairs_refit runs them."""
    for rec in V.segments()[4]:
        _clear_of_threshold(rec, 2.0, 300, 5, rounds)


def test_refit_summation_order_and_lstsq():
    """The refit does not depend on the order of the sums (the GPU's block
    reduction is one more permutation) and agrees with numpy's lstsq on the
    same normalised system, up to the f32 rounding of H: one ulp per entry
    moves a projection by about 5e-4 px at 640 px, so the bound is 1e-3 px."""
    rec, good = V.planted(300, 0.5, 5)
    _, mask, _ = V.verify(rec, 2.0, 256, 5, 0)
    a = V.refit(rec, mask)
    b = V.refit(rec, mask, order=np.random.default_rng(0).permutation(int(mask.sum())))
    pa, pb = V.project(a.reshape(3, 3), rec[:, :2]), V.project(b.reshape(3, 3), rec[:, :2])
    assert np.abs(pa - pb).max() < 1e-3
    cx, cy, s = V._box(rec[:, 0], rec[:, 1])
    CX, CY, S = V._box(rec[:, 2], rec[:, 3])
    r = rec[mask].astype(np.float64)
    rows, rhs = [], []
    for x, y, X, Y in zip((r[:, 0] - cx) * s, (r[:, 1] - cy) * s, (r[:, 2] - CX) * S, (r[:, 3] - CY) * S):
        rows += [[x, y, 1, 0, 0, 0, -X * x, -X * y], [0, 0, 0, x, y, 1, -Y * x, -Y * y]]
        rhs += [X, Y]
    g = np.linalg.lstsq(np.array(rows), np.array(rhs), rcond=None)[0]
    Tq = np.array([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1]])
    Tt = np.array([[S, 0, -S * CX], [0, S, -S * CY], [0, 0, 1]])
    pl = V.project(np.linalg.inv(Tt) @ np.append(g, 1.0).reshape(3, 3) @ Tq, rec[:, :2])
    assert np.abs(pa - pl).max() < 1e-3


# ---- each wrong variant is caught by a named fixture ------------------------------------
def test_variant_tie_high_and_repeat_on_four_matches():
    """m = 4: every valid hypothesis scores 4, so best_hypothesis is the first
    valid one; with replacement the first hypotheses repeat an index (area 0)
    and the first valid one comes later."""
    rec = V.four()
    want = V.verify(rec, 2.0, 64, 0, 0)[2]
    assert want["best_hypothesis"] == 0 and want["n_inliers"] == 4
    assert V.verify(rec, 2.0, 64, 0, 0, variant="tie_high")[2]["best_hypothesis"] == 63
    assert V.verify(rec, 2.0, 64, 0, 0, variant="repeat")[2]["best_hypothesis"] > 0


def test_variant_thr_lt_on_exact_translation():
    rec = V.translation_exact()
    H, mask, info = V.verify(rec, 2.0, 64, 0, 0)
    assert np.array_equal(H, np.array([[1, 0, 5], [0, 1, -3], [0, 0, 1]], np.float32))
    assert mask.all() and info["n_inliers"] == len(rec)
    _, mask_lt, info_lt = V.verify(rec, 2.0, 64, 0, 0, variant="thr_lt")
    assert not mask_lt[0] and mask_lt[1:].all() and info_lt["n_inliers"] == len(rec) - 1


def test_variant_no_orient_on_swapped_square():
    """Two swapped corners: every sample is twisted, so there is no model.
    Without the orientation test the four points still have an exact
    projective map; its line at infinity cuts the square, so w > 0 holds at
    two of the corners only: 2 inliers, a model nevertheless."""
    rec = V.square_swapped()
    assert V.verify(rec, 2.0, 64, 0, 0)[2] == dict(n_matches=4, n_inliers=0, best_hypothesis=-1, refits=0)
    info = V.verify(rec, 2.0, 64, 0, 0, variant="no_orient")[2]
    assert info["best_hypothesis"] == 0 and info["n_inliers"] == 2


# ---- ABI (no device needed) ----------------------------------------------------------------
def test_verify_null_context_rejected(pkg):
    from sift_features_amd import _lib
    L = pkg.lib()
    buf = (ctypes.c_uint8 * 256)()
    offs = (ctypes.c_size_t * 3)(0, 1, 2)
    po = (ctypes.c_size_t * 2)(0, 1)
    prm = _lib.RansacParams(3.0, 16, 0, 0)
    assert L.sift_mi_verify_pairs_device(None, buf, offs, 2, buf, 1, buf, po, ctypes.byref(prm), buf, buf) == -1
    assert L.sift_mi_verify_matches(None, buf, 1, buf, 1, buf, 1, ctypes.byref(prm), buf, buf) == -1
    assert b"null" in L.sift_mi_last_error()
    assert ctypes.sizeof(_lib.Homography) == 52 and ctypes.sizeof(_lib.RansacParams) == 16
