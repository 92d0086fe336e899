"""Pins prosac_ref.py, the restatement of the progressive (PROSAC) sampling
of the two geometric verifications, without a GPU: the draw function against
the siblings' samplers, the growth table by hand and by its properties, the
samples, the wrong variants on their fixtures, the invariance under the
caller's match order, and what the sampling is for: planted inliers at shares
where the uniform restatements give out."""
import functools

import numpy as np
import pytest

import epipolar_ref
import prosac_ref as P
import verify_ref

KS = {"homography": 4, "fundamental": 8}


def _result(r):
    g, mask, info = r
    return g.view(np.uint32).tolist(), mask.tolist(), info


# ---- the draw function -----------------------------------------------------------
@pytest.mark.parametrize("mod,k", [(verify_ref, 4), (epipolar_ref, 8)])
def test_draws_equal_the_siblings_samples(mod, k):
    hyps = np.concatenate([np.arange(300), [65535, 2**31 - 1, 2**32 - 1]])
    for seed in (0, 7, 0xFFFFFFFF):
        for m in (k, k + 1, 63, 400, 2**31 - 1):
            assert np.array_equal(P.draws(seed, hyps, m, k), mod.samples(seed, hyps, m)), (seed, m)
            # one bound per hypothesis, all the same
            assert np.array_equal(P.draws(seed, hyps, np.full(len(hyps), m), k), mod.samples(seed, hyps, m))


def test_draws_with_a_bound_per_hypothesis():
    hyps = np.arange(50)
    bound = 8 + hyps % 7
    got = P.draws(3, hyps, bound, 8)
    for h, b, row in zip(hyps, bound, got):
        assert np.array_equal(row, epipolar_ref.samples(3, [h], int(b))[0])


# ---- growth ------------------------------------------------------------------------
def test_growth_by_hand():
    """(N, k, T) = (10, 4, 1024): T_4 = 1024 / 210 = 4.876, T_5 = 24.38, T_6 =
    73.14, T_7 = 170.67, so the steps are ceil(19.50) = 20, ceil(48.76) = 49,
    ceil(97.52) = 98."""
    tp = P.growth(10, 4, 1024)
    assert tp[:5] == [0, 0, 0, 0, 1]
    assert (tp[5], tp[6], tp[7]) == (21, 70, 168)
    assert P.table(10, 4, 1024).tolist() == [0, 0, 0] + tp[4:]
    assert P.growth(3, 4, 1024) == [0, 0, 0, 0] and P.table(3, 4, 1024).tolist() == [0, 0, 0]


@pytest.mark.parametrize("k", [4, 8])
def test_growth_properties(k):
    for T in (1, 255, 1024, 65536):
        for N in list(range(k, k + 40)) + [63, 64, 400, 1025, 2049]:
            tp = P.growth(N, k, T)
            assert tp[k] == 1 and all(b > a for a, b in zip(tp[k:], tp[k + 1:])), (N, T)
            assert tp[N] <= T + N
            n = P.subset_size(np.arange(T if T < 4096 else 4096), N, k, T)
            assert n[0] == k and (np.diff(n) >= 0).all() and n.min() >= k and n.max() <= N + 1
    # the tail (n_h = N + 1) is reached when N is close to k
    for N in (k, k + 1):
        n = P.subset_size(np.arange(1024), N, k, 1024)
        assert (n == N + 1).any() and n[-1] == N + 1, N
    assert (P.subset_size(np.arange(1024), k, k, 1024)[1:] == k + 1).all()  # T'_k = 1: only hypothesis 0
    # no tail at 400 matches; the steps' ceil stretches the schedule a little (T'_N is about T + N - k), so the
    # last hypothesis draws from most of the set, not all of it
    n = P.subset_size(np.arange(1024), 400, k, 1024)
    assert 300 < n[-1] == n.max() <= 400


def test_growth_steps_of_one_for_a_huge_pair():
    """T_{n+1} - T_n = T_n k / (n + 1 - k) <= T k / (N - k) < 1 when N is near
    2^31 and T <= 65536: every step is ceil of a positive value below 1, so
    T'_n = n - k + 1 whatever the rounding (test_host_prosac.py holds the
    host table's last entry to it)."""
    for k in (4, 8):
        tp = P.growth(2**31 - 1, k, 65536, stop=k + 50)
        assert tp[k:] == list(range(1, 52))


# ---- samples -------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 8])
def test_samples_are_k_distinct_indices(k):
    for N in (k, k + 1, k + 2, 10, 63, 400):
        for T in (1, 64, 1024):
            hyps = np.arange(T)
            s = P.samples(5, hyps, N, k, T)
            assert s.shape == (T, k) and s.min() >= 0 and s.max() < N
            assert all(len(set(r)) == k for r in s.tolist())
            n = P.subset_size(hyps, N, k, T)
            prog = n <= N
            assert (s[prog, -1] == n[prog] - 1).all()  # the forced member
            assert (s[prog, :-1] < (n[prog] - 1)[:, None]).all()
            assert np.array_equal(s[~prog], P.draws(5, hyps[~prog], N, k))  # the uniform tail
    assert P.samples(0, [0], 400, k, 1024)[0].tolist()[-1] == k - 1 and set(P.samples(0, [0], 400, k, 1024)[0]) == set(range(k))


def test_the_siblings_are_left_as_they_were():
    before = verify_ref.samples, epipolar_ref.samples
    rec, _, q = P.value_fixture(*P.VALUE_CASES[2])
    P.verify(rec, q, "homography", 2.0, 64, 0, 0)
    with pytest.raises(ValueError):
        P.verify(rec, -q, "homography", 2.0, 64, 0, 0)
    assert (verify_ref.samples, epipolar_ref.samples) == before


def test_quality_checks():
    for bad in (np.nan, np.inf, -1.0, -0.0):
        with pytest.raises(ValueError):
            P.rank_order(np.array([1.0, bad, 2.0], np.float32))
    assert P.rank_order(np.array([3, 1, 3, 0, 1], np.float32)).tolist() == [3, 1, 4, 0, 2]
    assert P.rank_order(np.array([5, 5, 5], np.float32)).tolist() == [0, 1, 2]  # all equal: the identity


# ---- wrong variants ----------------------------------------------------------------------
@pytest.mark.parametrize("variant", P.VARIANTS)
def test_variant_changes_the_result_on_its_fixture(variant):
    rec, q, model, thr, it, seed = P.variant_fixture(variant)
    right = P.verify(rec, q, model, thr, it, seed, 0)
    wrong = P.verify(rec, q, model, thr, it, seed, 0, variant=variant)
    assert right[2]["best_hypothesis"] >= 0
    assert _result(right) != _result(wrong)
    if variant == "mask_rank":  # the same model and count, the mask in another order
        assert right[2] == wrong[2] and not np.array_equal(right[1], wrong[1])
    if variant == "no_tail":
        assert right[2]["best_hypothesis"] == 63 and right[2]["n_inliers"] == 6 and wrong[2]["n_inliers"] == 5
    if variant in ("le", "tn_200000"):  # boundary_twelve: the winner is the first hypothesis on the best seven
        tp = P.growth(12, 4, 256)
        assert tp[4:] == [1, 4, 10, 21, 40, 69, 113, 176, 262] and right[2]["best_hypothesis"] == tp[6]
        assert P.subset_size([tp[6]], 12, 4, 256).tolist() == [7]
        assert P.subset_size([tp[6]], 12, 4, 256, variant="le").tolist() == [6]
        # T_N = 200 000 stretches the schedule far past the call: its 256 hypotheses never leave the best five
        assert P.subset_size([tp[6], 255], 12, 4, 256, variant="tn_200000").tolist() == [5, 5]
    if variant in ("tie_high", "floor"):  # tied_triples: the boundaries run through equal qualities
        order, high = P.rank_order(q), P.rank_order(q, "tie_high")
        assert P.growth(60, 4, 64)[4:34] == list(range(1, 31))  # steps of one: every early boundary is used
        assert all(q[order[n - 1]] == q[order[n]] for n in range(4, 60) if n % 3)
        assert sorted(order[:4]) != sorted(high[:4])  # who is among the best four depends on the index
        assert set(P.growth(60, 4, 64, variant="floor")[4:34]) == {1}  # floor of a step below one: no growth


# ---- the caller's order --------------------------------------------------------------------
@pytest.mark.parametrize("model", ["homography", "fundamental"])
def test_permuting_the_matches_permutes_the_mask(model):
    rec, good = P.MODELS[model][0].planted(200, 0.5, 3)
    rng = np.random.default_rng(1)
    q = rng.permutation(200).astype(np.float32) + 1  # no ties
    g, mask, info = P.verify(rec, q, model, 2.0, 256, 3, 0)
    assert info["n_inliers"] >= 50
    perm = rng.permutation(200)
    g2, mask2, info2 = P.verify(rec[perm], q[perm], model, 2.0, 256, 3, 0)
    assert info2 == info and np.array_equal(g2.view(np.uint32), g.view(np.uint32))
    assert np.array_equal(mask2, mask[perm])


# ---- what it is for ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _value(case):
    model, m, share, seed = case
    rec, good, q = P.value_fixture(*case)
    uni = P.MODELS[model][0].verify(rec, 2.0, 1024, seed, 0)
    pro = P.verify(rec, q, model, 2.0, 1024, seed, 0)
    return good, uni, pro


@pytest.mark.parametrize("case", P.VALUE_CASES)
def test_progressive_recovers_what_uniform_misses(case):
    """400 matches, planted share 0.25 (fundamental) and 0.15 (homography),
    threshold 2.0, 1024 hypotheses, no refit: the uniform restatement recovers
    at most half of the planted inliers, the progressive one at least 95 %."""
    good, uni, pro = _value(case)
    n = int(good.sum())
    got_u, got_p = int((uni[1] & good).sum()), int((pro[1] & good).sum())
    print(f"{case}: planted {n}, uniform recovers {got_u}, progressive {got_p}")
    assert got_u <= 0.5 * n
    assert got_p >= 0.95 * n


def test_value_figures():
    """The figures the fixtures were fixed with."""
    got = [(int(g.sum()), int((u[1] & g).sum()), int((p[1] & g).sum())) for g, u, p in map(_value, P.VALUE_CASES)]
    assert got == [(103, 44, 102), (108, 51, 108), (56, 0, 56), (70, 16, 70)]


# ---- refit fixtures ------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.REFIT_CASES)
def test_refit_fixtures_stay_clear_of_the_threshold(case):
    """Every match is 1e-2 px from the threshold under every H / F a round
    scores, so the GPU's refit (sums in another order) gives the same masks."""
    model, m, share, seed = case
    rec, good, q = P.value_fixture(*case)
    for rounds in (1, 2):
        assert P.near_threshold_any(rec, q, model, 2.0, 512, seed, rounds) == []
        _, mask, info = P.verify(rec, q, model, 2.0, 512, seed, rounds)
        assert info["refits"] >= 1 and (mask & good).sum() >= 0.95 * good.sum()
