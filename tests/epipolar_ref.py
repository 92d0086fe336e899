"""numpy restatement of the epipolar verification of matched pairs (RANSAC
fundamental matrix, 8-point samples, Sampson score, eigen-refit on the
inliers) and the inputs its tests share (test_epipolar_ref_cpu.py pins it;
test_gpu_verify_epipolar.py holds the GPU path, csrc/verify_epipolar.hip,
against it).  LABELLED EXTENSION like verify_ref.py, whose sampling hash, box
normalisation and record helper it reuses.

A pair is m records (x, y, X, Y) f32: the query keypoint's position and the
train keypoint's.  F is row-major f[0..8] with (X, Y, 1) F (x, y, 1)^T = 0.
Every f64 / f32 step below is an elementwise expression with a stated operand
order (no @, np.dot or np.linalg inside the rule: BLAS may fuse).

    sampling   verify_ref's scheme with eight draws: s = mix32(mix32(seed +
               0x9E3779B9) ^ h); draw k = 0..7 is u = mix32(s + 0x85EBCA6B *
               (k + 1)), idx = (u * (m - k)) >> 32, then for each earlier pick
               in ascending order idx += (idx >= pick).  m < 8: no model.
    box        once per pair over ALL its matches (verify_ref._box, f64):
               x' = (x - cx) s_q, y' = (y - cy) s_q, X' = (X - CX) s_t,
               Y' = (Y - CY) s_t.
    model      f64, unfused.  A is 8 x 9, row i = [X'x', X'y', X', Y'x', Y'y',
               Y', x', y', 1] of sample i.  Gaussian elimination with complete
               pivoting: at step k the entry of largest |a[r][c]| over
               r = k..7, c = k..8, the first in row-major order on ties; a
               pivot equal to 0 makes the sample invalid; swap rows k, r and
               columns k, c; for each row r > k: f = a[r][k] / a[k][k],
               a[r][c] = a[r][c] - f a[k][c] for c > k.  Back substitution
               with g[8] = 1: for k = 7..0 s = -a[k][8], for c = k+1..7
               ascending s = s - a[k][c] g[c], g[k] = s / a[k][k]; the column
               permutation undone gives F'.  F = T_t^T F' T_q (_denorm), every
               entry divided by the entry of largest magnitude (the first in
               row-major order on ties, so that entry is exactly 1), rounded
               to f32.  Invalid unless the nine f32 values are finite; an
               invalid model is stored as nine zeros.  No rank-2 step, no
               degeneracy or orientation test.
    score      f32, unfused, no division: l0 = (f0 x + f1 y) + f2,
               l1 = (f3 x + f4 y) + f5, l2 = (f6 x + f7 y) + f8,
               m0 = (f0 X + f3 Y) + f6, m1 = (f1 X + f4 Y) + f7,
               e = (X l0 + Y l1) + l2, d = (l0 l0 + l1 l1) + (m0 m0 + m1 m1);
               inlier iff d > 0 and e e <= (thr thr) d: the Sampson distance
               <= thr px, NaN never an inlier.
    best       highest count among the valid hypotheses, lowest index on ties.
               m < 8 or no valid hypothesis: no model (f all 0, n_inliers 0,
               best_hypothesis -1, mask 0).
    refit      up to refit_rounds times; a round with fewer than 8 current
               inliers is rejected.  The 45 distinct sums of A^T A (rows as
               above, normalised coordinates) over the current inliers (SUMS),
               the eigenvector of its smallest eigenvalue by cyclic Jacobi
               (_jacobi: SWEEPS sweeps, p < q row-major, rotation skipped when
               a[p][q] == 0, smallest eigenvalue at the lowest index on ties);
               rank 2 by the same Jacobi on the 3 x 3 F'^T F': v its smallest
               eigenvector, F' <- F' - (F' v) v^T; denormalised, divided by the
               largest entry, rounded to f32, rescored.  The round is accepted
               iff the nine values are finite and the count did not drop; stop
               at the first rejected round or when the mask did not change
               (that round still counts as accepted).

So F is rank 2 (up to its f32 rounding) iff refits >= 1, the raw 8-point F
otherwise.  Known limits: a scene that is one plane satisfies a family of F
(the homography is the tool there), and an 8-point sample needs share^8 luck.

`variant` selects a deliberately wrong restatement (test use only): "tie_high"
highest index among equal counts, "thr_lt" a strict < in the inlier test,
"repeat" sampling with replacement, "one_sided" d = l0 l0 + l1 l1 only,
"no_colpivot" row pivoting only with the last column free (f'[8] = 1).
"""
import math

import numpy as np

from verify_ref import M32, _box, mix32, records  # noqa: F401  (records: re-exported for the tests)

VARIANTS = ("tie_high", "thr_lt", "repeat", "one_sided", "no_colpivot")
SWEEPS = 10  # cyclic Jacobi sweeps (test_jacobi_matches_eigh fixes the count)


# ---- sampling ---------------------------------------------------------------
def samples(seed, hyps, m, variant=None):
    """(len(hyps), 8) int64 indices into the pair's m >= 8 matches."""
    h = np.asarray(hyps, np.uint64)
    s = mix32(mix32((int(seed) + 0x9E3779B9) & M32) ^ h)
    picks = []
    for k in range(8):
        u = mix32((s + np.uint64((0x85EBCA6B * (k + 1)) & M32)) & M32)
        if variant == "repeat":
            picks.append(((u * np.uint64(m)) >> np.uint64(32)).astype(np.int64))
            continue
        idx = ((u * np.uint64(m - k)) >> np.uint64(32)).astype(np.int64)
        if picks:
            earlier = np.sort(np.stack(picks, 1), axis=1)
            for j in range(k):
                idx = idx + (idx >= earlier[:, j])
        picks.append(idx)
    return np.stack(picks, 1)


# ---- model ------------------------------------------------------------------
def box(rec):
    """(cx, cy, s_q, CX, CY, s_t) f64 of the records' box normalisation."""
    rec = np.asarray(rec, np.float32)
    return _box(rec[:, 0], rec[:, 1]) + _box(rec[:, 2], rec[:, 3])


def _rows(x, y, X, Y):
    """The nine entries of a row of A (normalised f64 coordinates)."""
    return [X * x, X * y, X, Y * x, Y * y, Y, x, y, np.ones_like(x)]


def _normalise(r, bx):
    cx, cy, sq, CX, CY, st = bx
    return (r[..., 0] - cx) * sq, (r[..., 1] - cy) * sq, (r[..., 2] - CX) * st, (r[..., 3] - CY) * st


def _denorm(fp, bx):
    """F = T_t^T F' T_q for F' fp[r][c] (arrays or floats), T_q = [[s_q, 0, -s_q cx], [0, s_q, -s_q cy], [0, 0, 1]]
    and T_t the same on the train side: G = F' T_q, then F = T_t^T G."""
    cx, cy, sq, CX, CY, st = bx
    G = []
    for r in range(3):
        g0, g1 = fp[r][0] * sq, fp[r][1] * sq
        G.append([g0, g1, fp[r][2] - (g0 * cx + g1 * cy)])
    F0 = [G[0][c] * st for c in range(3)]
    F1 = [G[1][c] * st for c in range(3)]
    F2 = [G[2][c] - (F0[c] * CX + F1[c] * CY) for c in range(3)]
    return [F0, F1, F2]


def _scale_f32(F):
    """(n, 9) f64 -> every row divided by its entry of largest magnitude (first on ties), as f32."""
    mag = np.abs(F)
    mag = np.where(np.isnan(mag), -1.0, mag)
    big = F[np.arange(len(F)), np.argmax(mag, 1)]
    return (F / big[:, None]).astype(np.float32)


def models(rec, seed, hyps, variant=None):
    """F (n, 9) f32 (zeros where invalid) and validity (n,) bool of hypotheses `hyps` on rec (m >= 8, 4) f32."""
    rec = np.asarray(rec, np.float32)
    bx = box(rec)
    idx = samples(seed, hyps, len(rec), variant)
    n = len(idx)
    ar = np.arange(n)
    a = np.stack(_rows(*_normalise(rec[idx].astype(np.float64), bx)), 2)  # (n, 8 samples, 9)
    perm = np.tile(np.arange(9), (n, 1))
    valid = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for k in range(8):
            if variant == "no_colpivot":
                mag = np.abs(a[:, k:, k])
                r, c = k + np.argmax(np.where(np.isnan(mag), -1.0, mag), 1), np.full(n, k)
            else:
                mag = np.abs(a[:, k:, k:]).reshape(n, -1)
                j = np.argmax(np.where(np.isnan(mag), -1.0, mag), 1)
                r, c = k + j // (9 - k), k + j % (9 - k)
            valid &= a[ar, r, c] != 0
            t = a[ar, k].copy()
            a[ar, k] = a[ar, r]
            a[ar, r] = t
            t = a[ar, :, k].copy()
            a[ar, :, k] = a[ar, :, c]
            a[ar, :, c] = t
            t = perm[ar, k].copy()
            perm[ar, k] = perm[ar, c]
            perm[ar, c] = t
            for r_ in range(k + 1, 8):
                f = a[:, r_, k] / a[:, k, k]
                for c_ in range(k + 1, 9):
                    a[:, r_, c_] = a[:, r_, c_] - f * a[:, k, c_]
        g = [None] * 8 + [np.ones(n)]
        for k in range(7, -1, -1):
            s = -a[:, k, 8]
            for c_ in range(k + 1, 8):
                s = s - a[:, k, c_] * g[c_]
            g[k] = s / a[:, k, k]
        fp = np.zeros((n, 9))
        for j in range(9):
            fp[ar, perm[:, j]] = g[j]
        F = _denorm([[fp[:, 3 * r_ + c_] for c_ in range(3)] for r_ in range(3)], bx)
        f = _scale_f32(np.stack([F[r_][c_] for r_ in range(3) for c_ in range(3)], 1))
    valid &= np.isfinite(f).all(1)
    f[~valid] = 0
    return f, valid


# ---- score ------------------------------------------------------------------
def inlier_mask(rec, f, thr, variant=None):
    """rec (m, 4) f32; f (9,) or (n, 9) f32 -> bool (m,) or (n, m)."""
    rec = np.asarray(rec, np.float32)
    f = np.asarray(f, np.float32)
    g = f.reshape(-1, 9)[:, :, None]
    x, y, X, Y = (rec[None, :, k] for k in range(4))
    thr = np.float32(thr)
    with np.errstate(all="ignore"):
        l0 = (g[:, 0] * x + g[:, 1] * y) + g[:, 2]
        l1 = (g[:, 3] * x + g[:, 4] * y) + g[:, 5]
        l2 = (g[:, 6] * x + g[:, 7] * y) + g[:, 8]
        m0 = (g[:, 0] * X + g[:, 3] * Y) + g[:, 6]
        m1 = (g[:, 1] * X + g[:, 4] * Y) + g[:, 7]
        e = (X * l0 + Y * l1) + l2
        d = (l0 * l0 + l1 * l1) if variant == "one_sided" else (l0 * l0 + l1 * l1) + (m0 * m0 + m1 * m1)
        ee, lim = e * e, (thr * thr) * d
        ok = (d > 0) & ((ee < lim) if variant == "thr_lt" else (ee <= lim))
    assert e.dtype == np.float32 and d.dtype == np.float32
    return ok[0] if f.ndim == 1 else ok


# ---- refit ------------------------------------------------------------------
TERMS = ("Xx", "Xy", "X", "Yx", "Yy", "Y", "x", "y", "1")
# the 45 distinct sums of A^T A, upper triangle row by row: "Xx.Xy" is the sum of (X x) (X y)
SUMS = tuple(f"{TERMS[j]}.{TERMS[k]}" for j in range(9) for k in range(j, 9))


def _jacobi(a, sweeps=SWEEPS):
    """Cyclic Jacobi on the symmetric n x n `a` (lists of Python floats, changed
    in place) -> (eigenvalues = its diagonal, V with the eigenvectors in its
    columns)."""
    n = len(a)
    v = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    for _ in range(sweeps):
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = a[p][q]
                if apq == 0.0:
                    continue
                theta = (a[q][q] - a[p][p]) / (2.0 * apq)
                t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(n):
                    if k != p and k != q:
                        akp, akq = a[k][p], a[k][q]
                        a[k][p] = a[p][k] = c * akp - s * akq
                        a[k][q] = a[q][k] = s * akp + c * akq
                a[p][p] = a[p][p] - t * apq
                a[q][q] = a[q][q] + t * apq
                a[p][q] = a[q][p] = 0.0
                for k in range(n):
                    vkp, vkq = v[k][p], v[k][q]
                    v[k][p] = c * vkp - s * vkq
                    v[k][q] = s * vkp + c * vkq
    return [a[i][i] for i in range(n)], v


def _smallest(a, sweeps=SWEEPS):
    """The eigenvector of the smallest eigenvalue (lowest index on ties) of the symmetric `a`."""
    w, v = _jacobi(a, sweeps)
    j = 0
    for i in range(1, len(w)):
        if w[i] < w[j]:
            j = i
    return [v[i][j] for i in range(len(w))]


def moments(rec, mask, order=None):
    """The 9 x 9 A^T A (lists of floats) of the inliers `mask`, summed sequentially in `order`."""
    rec = np.asarray(rec, np.float32)
    r = rec[np.asarray(mask, bool)].astype(np.float64)
    if order is not None:
        r = r[order]
    t = _rows(*_normalise(r, box(rec)))
    sums = {}
    for j in range(9):
        for k in range(j, 9):
            acc = 0.0
            for e in t[j] * t[k]:  # sequential: the order is part of what `order` permutes
                acc = acc + float(e)
            sums[f"{TERMS[j]}.{TERMS[k]}"] = acc
    assert tuple(sums) == SUMS
    return [[sums[f"{TERMS[min(j, k)]}.{TERMS[max(j, k)]}"] for k in range(9)] for j in range(9)]


def refit(rec, mask, order=None, f64=False):
    """One least-squares rank-2 F (9,) f32 on the inliers `mask` (not rescored); None with fewer than 8 of them.
    `order` permutes the summation; `f64` returns the scaled F before its rounding."""
    rec = np.asarray(rec, np.float32)
    if int(np.asarray(mask, bool).sum()) < 8:
        return None
    with np.errstate(all="ignore"):
        f = _smallest(moments(rec, mask, order))
        fp = [[f[3 * r + c] for c in range(3)] for r in range(3)]
        mm = [[(fp[0][i] * fp[0][j] + fp[1][i] * fp[1][j]) + fp[2][i] * fp[2][j] for j in range(3)] for i in range(3)]
        v = _smallest(mm)
        fv = [(fp[r][0] * v[0] + fp[r][1] * v[1]) + fp[r][2] * v[2] for r in range(3)]
        fp = [[fp[r][c] - fv[r] * v[c] for c in range(3)] for r in range(3)]
        F = _denorm(fp, box(rec))
        F = np.array([[F[r][c] for r in range(3) for c in range(3)]], np.float64)
        if f64:
            mag = np.abs(F[0])
            return F[0] / F[0][np.argmax(np.where(np.isnan(mag), -1.0, mag))]
        return _scale_f32(F)[0]


# ---- the whole rule ---------------------------------------------------------
def verify(rec, threshold=3.0, iterations=1024, seed=0, refit_rounds=2, variant=None, trace=None):
    """-> (F (3, 3) f32, mask (m,) bool, info dict n_matches / n_inliers / best_hypothesis / refits).
    `trace`, a list, receives every F (9,) a refit round scored, accepted or not."""
    rec = np.asarray(rec, np.float32).reshape(-1, 4)
    m = len(rec)
    none = (np.zeros((3, 3), np.float32), np.zeros(m, bool),
            dict(n_matches=m, n_inliers=0, best_hypothesis=-1, refits=0))
    if m < 8:
        return none
    best, best_n, best_f = -1, -1, None
    for h0 in range(0, iterations, 256):
        hyps = np.arange(h0, min(h0 + 256, iterations))
        f, valid = models(rec, seed, hyps, variant)
        cnt = inlier_mask(rec, f, threshold, variant).sum(1)
        for i in np.nonzero(valid)[0]:
            if cnt[i] > best_n or (variant == "tie_high" and cnt[i] == best_n):
                best, best_n, best_f = int(hyps[i]), int(cnt[i]), f[i]
    if best < 0:
        return none
    mask = inlier_mask(rec, best_f, threshold, variant)
    refits = 0
    for _ in range(refit_rounds):
        f2 = refit(rec, mask)
        if f2 is None or not np.isfinite(f2).all():
            break
        if trace is not None:
            trace.append(f2)
        mask2 = inlier_mask(rec, f2, threshold, variant)
        if mask2.sum() < mask.sum():
            break
        same = np.array_equal(mask, mask2)
        best_f, mask, refits = f2, mask2, refits + 1
        if same:
            break
    return best_f.reshape(3, 3).copy(), mask, dict(n_matches=m, n_inliers=int(mask.sum()), best_hypothesis=best,
                                                   refits=refits)


def sampson(rec, f):
    """f64 Sampson distances (px) of the records under f (3, 3); inf where the gradient vanishes."""
    rec = np.asarray(rec, np.float64)
    f = np.asarray(f, np.float64).reshape(3, 3)
    q = np.concatenate([rec[:, :2], np.ones((len(rec), 1))], 1)
    t = np.concatenate([rec[:, 2:4], np.ones((len(rec), 1))], 1)
    l, mm = q @ f.T, t @ f
    e = (t * l).sum(1)
    d = l[:, 0] ** 2 + l[:, 1] ** 2 + mm[:, 0] ** 2 + mm[:, 1] ** 2
    with np.errstate(all="ignore"):
        return np.where(d > 0, np.abs(e) / np.sqrt(d), np.inf)


# ---- fixtures ---------------------------------------------------------------
K_CAM = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


R_MILD, T_MILD = _rot(0.01, -0.03, 0.015), np.array([0.35, 0.05, 0.1])


def true_f(R=R_MILD, t=T_MILD, K=K_CAM):
    """F = K^-T [t]x R K^-1 of the second camera (R, t) against the first."""
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    return Ki.T @ tx @ R @ Ki


def two_view(q, depth, R=R_MILD, t=T_MILD, K=K_CAM):
    """Train pixels (n, 2) f64 of the query pixels q (n, 2) at the given depths."""
    P = (np.linalg.inv(K) @ np.concatenate([q, np.ones((len(q), 1))], 1).T) * depth
    p = K @ (R @ P + t[:, None])
    return (p[:2] / p[2]).T


def planted(m, inlier_share, seed, R=R_MILD, t=T_MILD):
    """m records of a two-view scene: query points uniform in 640 x 480 at
    depths 4..12, seen by a second camera a small rotation and a translation
    away, with +-0.5 px uniform noise (the planted inliers); the rest go to
    uniform-random train points.  Train points are clipped to 640 x 480; a
    planted inlier the clip moved is not counted as planted.
    -> (rec f32, planted mask)."""
    rng = np.random.default_rng(seed)
    q = rng.uniform([20, 20], [620, 460], (m, 2))
    tr = two_view(q, rng.uniform(4.0, 12.0, m), R, t) + rng.uniform(-0.5, 0.5, (m, 2))
    good = rng.random(m) < inlier_share
    tr[~good] = rng.uniform([0, 0], [640, 480], (int((~good).sum()), 2))
    clipped = np.clip(tr, [0, 0], [640, 480])
    good &= (clipped == tr).all(1)
    return np.concatenate([q, clipped], 1).astype(np.float32), good


# (m, planted share, seed) of the fixtures the refit tests use, on the GPU too
# (threshold 2.0, 512 hypotheses, seed = the fixture's)
REFIT_CASES = [(300, 0.6, 0), (300, 0.5, 5), (65, 0.7, 2), (1030, 0.6, 3), (9, 1.0, 4)]

# as verify_ref.SEG_MATCHES, with the small pairs around the 8-match minimum
SEG_MATCHES = [0, 300, 7, 0, 1030, 64, 8, 200, 0]
SEG_TWICE = 1
SEG_SEED = 21


def segments(seed=SEG_SEED):
    """One keypoint arena for SEG_MATCHES, built as verify_ref.segments()
    builds its own: pair p matches segment 2p (query) against segment 2p + 1
    (train), every pair planted with the same two-view scene (60 % inliers),
    so a read past a pair's records finds inliers of the same F and raises
    n_inliers.  -> (kps (n, 5) f32, offsets, pairs, matches per pair, records
    per pair)."""
    rng = np.random.default_rng(seed)
    kps, offs, pairs, matches, recs = [], [0], [], [], []
    for p, m in enumerate(SEG_MATCHES):
        rec = planted(m, 0.6, seed + p)[0]
        idx = []
        for cols in (slice(0, 2), slice(2, 4)):
            n = m + 3 if m else (0 if p == 0 else 2)  # the first pair's segments are empty as well
            pos = rng.permutation(n)[:m]
            k = np.zeros((n, 5), np.float32)
            k[:, :2] = rng.uniform(0, 480, (n, 2))
            k[pos, :2] = rec[:, cols]
            k[:, 2:] = rng.uniform(1, 5, (n, 3))
            kps.append(k)
            offs.append(offs[-1] + n)
            idx.append(pos.astype(np.int32))
        pairs.append((2 * p, 2 * p + 1))
        matches.append((idx[0], idx[1], np.zeros(m, np.float32)))
        recs.append(rec)
    pairs.append(pairs[SEG_TWICE])
    matches.append(matches[SEG_TWICE])
    recs.append(recs[SEG_TWICE])
    return np.concatenate(kps), np.asarray(offs, np.int64), pairs, matches, recs


def eight_exact(seed=5):
    """m = 8 noise-free matches of the two-view scene: every hypothesis draws
    the same eight matches (in another order), and each scores 8."""
    rng = np.random.default_rng(seed)
    q = rng.uniform([20, 20], [620, 460], (8, 2))
    return np.concatenate([q, two_view(q, rng.uniform(4.0, 12.0, 8))], 1).astype(np.float32)


def threshold_exact(thr=3.0, seed=7, m=40):
    """Integer coordinates with y = 3k, Y = 4k (k in 0..64, both ends present)
    and x, X integers in 0..256 (0 and 256 present), so both box scales are
    2^-7 and F is proportional to [[0,0,0],[0,0,-.75],[0,1,0]] (e = y - .75 Y);
    match 0 has Y lowered by 5, which puts it at exactly thr = 3: e = 3.75,
    d = 1 + .75^2, e e == thr^2 d in f32."""
    assert thr == 3.0
    rng = np.random.default_rng(seed)
    k = np.concatenate([[32, 0, 64], rng.integers(1, 64, m - 3)]).astype(np.float64)
    x = np.concatenate([[100, 0, 256], rng.integers(0, 257, m - 3)]).astype(np.float64)
    X = np.concatenate([[37, 256, 0], rng.integers(0, 257, m - 3)]).astype(np.float64)
    rec = np.stack([x, 3 * k, X, 4 * k], 1)
    rec[0, 3] -= 5
    return rec.astype(np.float32)


def sideways(m=40, seed=9):
    """A pure sideways translation seen by identical cameras: Y = y, integer
    coordinates whose boxes are both 0..256 squared (the corners are present),
    so y' and Y' are the same bits and F is [[0,0,0],[0,0,1],[0,-1,0]] up to
    sign, with f[8] = 0: complete pivoting leaves one of the two equal columns
    free, while the rows-only elimination with the last column free has no
    solution to find (its last pivots are zero or rounding residue)."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([[0, 256], rng.integers(0, 257, m - 2)])
    y = np.concatenate([[256, 0], rng.integers(0, 257, m - 2)])
    X = np.concatenate([[256, 0], rng.integers(0, 257, m - 2)])
    return np.stack([x, y, X, y], 1).astype(np.float32)


def near_threshold(rec, f, thr, margin=1e-2):
    """Indices of the matches whose f64 Sampson distance under f lies within `margin` px of thr."""
    return np.nonzero(np.abs(sampson(rec, f) - thr) < margin)[0]


def near_threshold_any(rec, thr, iterations, seed, refit_rounds, margin=1e-2):
    """The same under the final F of verify(...) and under every F one of its
    refit rounds scored, accepted or rejected: empty means that every mask and
    every accept / reject decision has `margin` px to spare."""
    trace = []
    F, _, info = verify(rec, thr, iterations, seed, refit_rounds, trace=trace)
    fs = ([F] if info["best_hypothesis"] >= 0 else []) + [t.reshape(3, 3) for t in trace]
    return sorted({int(i) for f in fs for i in near_threshold(rec, f, thr, margin)})
