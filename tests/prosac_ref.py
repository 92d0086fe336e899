"""numpy restatement of the progressive (PROSAC) sampling of the two geometric
verifications (test_prosac_ref_cpu.py pins it; test_gpu_verify_progressive.py
holds the GPU path, the *_progressive calls of csrc/verify.hip and
csrc/verify_epipolar.hip, against it).  LABELLED EXTENSION like verify_ref.py
and epipolar_ref.py, whose solves, scores and refits it runs unchanged: only
the order of a pair's records and the indices a hypothesis draws differ.

Chum & Matas, "Matching with PROSAC - progressive sample consensus", CVPR
2005.  k is 4 (homography) or 8 (fundamental matrix), N the pair's match count,
T the call's `iterations`.

    rank       match i has the key (u32 pattern of quality[i], i); quality is
               f32, finite, sign bit clear, so the pattern orders as the value.
               The records are put in ascending key order: lower quality
               value first (a descriptor distance: lower is better), lower
               index first among equals.
    growth     f64, one rounding per operation, no fused multiply-add.
               T_k = T; for i = 0..k-1 in that order T_k = T_k * (k - i) /
               (N - i), multiply then divide.  T_{n+1} = T_n * (n + 1) /
               (n + 1 - k).  T'_k = 1, T'_{n+1} = T'_n + ceil(T_{n+1} - T_n),
               integers.  The paper fixes T_N = 200 000 draws; here T_N is the
               call's own `iterations`, so the schedule reaches the whole set
               as the call ends (a pair of ten matches is not sampled from its
               top five a thousand times).
    sample     of hypothesis h (0-based): n_h is the smallest n in [k, N] with
               h < T'_n.  If there is one: the k - 1 draws of the siblings'
               scheme below n_h - 1 (draws(seed, h, n_h - 1, k - 1)) in draw
               order, then rank n_h - 1 as the last member.  Otherwise (h >=
               T'_N: the tail, reached when N is close to k) the siblings' k
               draws below N, over the ranked records.  The hash is theirs.
    the rest   verify_ref.verify / epipolar_ref.verify on the ranked records:
               validity, the f64 minimal solve, the f32 score, the lowest
               hypothesis among equal counts, "no model", the refit rounds.
               best_hypothesis is the hypothesis index; the mask is reported
               in the caller's match order.

PROSAC's own stopping criteria (non-randomness, maximality) are not part of
the rule: all hypotheses of a call run at once.

`variant` selects a deliberately wrong restatement (test use only):
"worst_first" descending keys, "tie_high" higher index first among equal
quality, "no_forced" k draws from the top n_h without the forced member,
"le" h <= T'_n, "floor" floor for ceil, "tn_200000" the paper's fixed T_N,
"no_tail" n = N with a forced last member in the tail, "mask_rank" the mask
left in rank order.
"""
import math

import numpy as np

import epipolar_ref
import verify_ref
from verify_ref import M32, mix32

VARIANTS = ("worst_first", "tie_high", "no_forced", "le", "floor", "tn_200000", "no_tail", "mask_rank")
MODELS = {"homography": (verify_ref, 4), "fundamental": (epipolar_ref, 8)}


# ---- rank ---------------------------------------------------------------------
def check_quality(quality):
    """f32 array of the qualities; ValueError where the C ABI answers SIFT_MI_EINVAL."""
    q = np.ascontiguousarray(quality, np.float32).reshape(-1)
    if not np.isfinite(q).all():
        raise ValueError("quality must be finite")
    if (q.view(np.uint32) >> np.uint32(31)).any():
        raise ValueError("quality must have its sign bit clear")
    return q


def rank_order(quality, variant=None):
    """order[r] = the caller's index of the match at rank r."""
    bits = check_quality(quality).view(np.uint32).astype(np.int64)
    idx = np.arange(len(bits), dtype=np.int64)
    if variant == "worst_first":
        return np.lexsort((-idx, -bits))
    if variant == "tie_high":
        return np.lexsort((-idx, bits))
    return np.lexsort((idx, bits))


# ---- growth -------------------------------------------------------------------
def growth(N, k, T, variant=None, stop=None):
    """T'_n for n = 0..min(N, stop) as a list of ints (0 below n = k); [] .. all 0 when N < k."""
    last = N if stop is None else min(N, stop)
    tp = [0] * (last + 1)
    if N < k:
        return tp
    t = 200000.0 if variant == "tn_200000" else float(T)
    for i in range(k):
        t = t * float(k - i)
        t = t / float(N - i)
    tp[k] = 1
    for n in range(k, last):
        t1 = t * float(n + 1)
        t1 = t1 / float(n + 1 - k)
        d = t1 - t
        tp[n + 1] = tp[n] + (math.floor(d) if variant == "floor" else math.ceil(d))
        t = t1
    return tp


def table(N, k, T):
    """The host's u32 slice of a pair: T'_{i + 1} at rank position i >= k - 1, 0 below."""
    tp = growth(N, k, T)
    return np.array([tp[i + 1] if i >= k - 1 else 0 for i in range(N)], np.uint32)


# ---- sample -------------------------------------------------------------------
def draws(seed, hyps, bound, k, variant=None):
    """(len(hyps), k) int64: the siblings' k distinct draws below bound >= k,
    a scalar or one bound per hypothesis."""
    h = np.asarray(hyps, np.uint64)
    bound = np.broadcast_to(np.asarray(bound, np.int64), h.shape)
    s = mix32(mix32((int(seed) + 0x9E3779B9) & M32) ^ h)
    picks = []
    for j in range(k):
        u = mix32((s + np.uint64((0x85EBCA6B * (j + 1)) & M32)) & M32)
        idx = ((u * (bound - j).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        if picks:
            earlier = np.sort(np.stack(picks, 1), axis=1)
            for i in range(j):
                idx = idx + (idx >= earlier[:, i])
        picks.append(idx)
    return np.stack(picks, 1) if picks else np.zeros((len(h), 0), np.int64)


def subset_size(hyps, N, k, T, variant=None):
    """n_h per hypothesis; N + 1 marks the tail."""
    tp = np.asarray(growth(N, k, T, variant)[k:], np.int64)  # T'_k .. T'_N
    h = np.asarray(hyps, np.int64)
    if variant == "floor":  # not ascending: the first n with h < T'_n, by a scan
        ok = h[:, None] < tp[None, :]
        first = np.where(ok.any(1), ok.argmax(1), len(tp))
    else:
        first = np.searchsorted(tp, h, side="left" if variant == "le" else "right")
    return first + k


def samples(seed, hyps, N, k, T, variant=None):
    """(len(hyps), k) int64 rank positions of the progressive samples of a pair of N >= k matches."""
    h = np.asarray(hyps, np.int64)
    n = subset_size(h, N, k, T, variant)
    tail = n > N
    uniform = draws(seed, h, N, k)
    if variant == "no_tail":
        n, tail = np.minimum(n, N), np.zeros(len(h), bool)
    nn = np.where(tail, N, n)
    if variant == "no_forced":
        prog = draws(seed, h, nn, k)
    else:
        prog = np.concatenate([draws(seed, h, nn - 1, k - 1), (nn - 1)[:, None]], 1)
    return np.where(tail[:, None], uniform, prog)


# ---- the whole rule -----------------------------------------------------------
def verify(rec, quality, model="homography", threshold=3.0, iterations=1024, seed=0, refit_rounds=2, variant=None,
           trace=None):
    """-> (H or F (3, 3) f32, mask (m,) bool in the caller's order, info) as the sibling's verify()."""
    mod, k = MODELS[model]
    rec = np.asarray(rec, np.float32).reshape(-1, 4)
    order = rank_order(quality, variant)
    if len(order) != len(rec):
        raise ValueError("one quality per match")

    def progressive(seed_, hyps, m, variant_=None):
        return samples(seed_, hyps, m, k, iterations, variant)

    saved = mod.samples
    mod.samples = progressive
    try:
        g, mask_r, info = mod.verify(rec[order], threshold, iterations, seed, refit_rounds, trace=trace)
    finally:
        mod.samples = saved
    if variant == "mask_rank":
        return g, mask_r, info
    mask = np.zeros(len(rec), bool)
    mask[order] = mask_r
    return g, mask, info


def near_threshold_any(rec, quality, model, thr, iterations, seed, refit_rounds, margin=1e-2):
    """The sibling's near_threshold_any under the progressive rule: the matches
    within `margin` px of thr under the final model or under any model a refit
    round scored."""
    mod, _ = MODELS[model]
    trace = []
    g, _, info = verify(rec, quality, model, thr, iterations, seed, refit_rounds, trace=trace)
    gs = ([g] if info["best_hypothesis"] >= 0 else []) + [t.reshape(3, 3) for t in trace]
    return sorted({int(i) for m_ in gs for i in mod.near_threshold(rec, m_, thr, margin)})


# ---- fixtures -----------------------------------------------------------------
def synthetic_quality(good, seed):
    """A descriptor-distance-like quality: inliers from N(150, 50), outliers
    from N(260, 60), clipped at 1 and rounded (so there are ties), f32."""
    rng = np.random.default_rng(100 + seed)
    q = np.where(good, rng.normal(150.0, 50.0, len(good)), rng.normal(260.0, 60.0, len(good)))
    return np.round(np.maximum(q, 1.0)).astype(np.float32)


# (model, m, planted share, seed) of the value test: threshold 2.0, 1024
# hypotheses, seed = the fixture's, no refit, synthetic_quality(planted, seed)
VALUE_CASES = [("fundamental", 400, 0.25, 0), ("fundamental", 400, 0.25, 1),
               ("homography", 400, 0.15, 1), ("homography", 400, 0.15, 2)]


def value_fixture(model, m, share, seed):
    """-> (rec, planted mask, quality) of a VALUE_CASES entry."""
    rec, good = MODELS[model][0].planted(m, share, seed)
    return rec, good, synthetic_quality(good, seed)


def tail_six():
    """Six noisy inliers of verify_ref.H_MILD ranked in their own order, for
    64 hypotheses at threshold 0.5 with seed 5: T' = 1, 19, 62, so hypotheses
    62 and 63 are the tail.  The rule's winner is the uniform draw of
    hypothesis 63 with all six as inliers; with a forced last member there no
    hypothesis finds more than five (the winner is hypothesis 2)."""
    return verify_ref.planted(6, 1.0, 5)[0], np.arange(6, dtype=np.float32)


def boundary_twelve():
    """Twelve matches (verify_ref.planted(12, 0.6, 7), synthetic quality) for
    256 hypotheses at threshold 1.0 with seed 7: T' = 1, 4, 10, 21, 40, 69,
    113, 176, 262.  The rule's winner is hypothesis 10 = T'_6, the first that
    draws from the best seven; `h <= T'_n` keeps it on the best six, and with
    T_N fixed at 200 000 the schedule is so long that none of the 256
    hypotheses leaves the best five."""
    rec, good = verify_ref.planted(12, 0.6, 7)
    return rec, synthetic_quality(good, 7)


def tied_triples():
    """Sixty matches (verify_ref.planted(60, 0.5, 0)) whose qualities are 0, 0,
    0, 1, 1, 1, ... along the synthetic quality's order, scattered over the
    caller's order, for 64 hypotheses at threshold 2.0 with seed 0: T'_n = n -
    3 up to n = 33, every step the ceil of a value below one, and every n_h
    boundary that is no multiple of three runs through equal qualities, so
    the index decides who is inside.  With `floor` none of those steps is
    taken."""
    rec, good = verify_ref.planted(60, 0.5, 0)
    order = np.argsort(synthetic_quality(good, 0), kind="stable")
    q = np.empty(60, np.float32)
    q[order] = (np.arange(60) // 3).astype(np.float32)
    return rec, q


# variant -> (fixture, model, threshold, iterations, seed); "value" is VALUE_CASES[3]
VARIANT_FIXTURES = {"worst_first": ("value", "homography", 2.0, 1024, 2), "tie_high": ("tied_triples", "homography", 2.0, 64, 0),
                    "no_forced": ("value", "homography", 2.0, 1024, 2), "le": ("boundary_twelve", "homography", 1.0, 256, 7),
                    "floor": ("tied_triples", "homography", 2.0, 64, 0),
                    "tn_200000": ("boundary_twelve", "homography", 1.0, 256, 7),
                    "no_tail": ("tail_six", "homography", 0.5, 64, 5), "mask_rank": ("value", "homography", 2.0, 1024, 2)}


def variant_fixture(variant):
    """-> (rec, quality, model, threshold, iterations, seed) on which `variant` changes the result."""
    name, *rest = VARIANT_FIXTURES[variant]
    if name == "value":
        rec, _, q = value_fixture(*VALUE_CASES[3])
    else:
        rec, q = {"tail_six": tail_six, "boundary_twelve": boundary_twelve, "tied_triples": tied_triples}[name]()
    return (rec, q, *rest)


# (model, m, planted share, seed) of the fixtures the refit tests use, on the
# GPU too (threshold 2.0, 512 hypotheses, seed = the fixture's,
# synthetic_quality of the planted mask)
REFIT_CASES = [("homography", 300, 0.3, 0), ("homography", 1030, 0.5, 4), ("homography", 65, 0.6, 3),
               ("fundamental", 300, 0.5, 5), ("fundamental", 65, 0.7, 2), ("fundamental", 1030, 0.6, 3)]
