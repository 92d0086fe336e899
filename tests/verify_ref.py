"""numpy restatement of the geometric verification of matched pairs (RANSAC
homography, inlier refit) and the inputs its tests share
(test_verify_ref_cpu.py pins it; test_gpu_verify.py holds the GPU path,
csrc/verify.hip, against it).  LABELLED EXTENSION: the crate has nothing like
it (examples/sift-match.rs stops at drawing the matches).

A pair is m records (x, y, X, Y) f32: the query keypoint's position and the
train keypoint's.  H maps (x, y, 1) to (X, Y, 1), row-major, h[8] == 1.

    sampling   u32 arithmetic only.  mix32(x): x ^= x >> 16; x *= 0x7feb352d;
               x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.  Hypothesis h has
               s = mix32(mix32(seed + 0x9E3779B9) ^ h); draw k = 0..3 is
               u = mix32(s + 0x85EBCA6B * (k + 1)), idx = (u * (m - k)) >> 32
               (64-bit product), then for each earlier pick in ascending
               order idx += (idx >= pick): four distinct indices, no loop.
               The pair's place in the call is not an input.
    validity   f64 from the f32 coordinates.  The doubled signed area
               (bx - ax) * (cy - ay) - (by - ay) * (cx - ax) of the triples
               (0,1,2) (0,1,3) (0,2,3) (1,2,3) of the sample, in the query and
               in the train image: invalid if any is 0 or if the two signs of
               a triple differ (a twisted quadrilateral).
    model      f64, unfused.  M = [[x1,x2,x3],[y1,y2,y3],[1,1,1]],
               lambda = adj(M) (x4, y4, 1), basis = M diag(lambda); A from the
               query points, B from the train points, H = B adj(A), H /= H[2][2]
               and rounded to f32.  Invalid unless the nine f32 values are
               finite.  adj() and the products' operand order: _adj, _mat3.
    score      f32, unfused: w = (h6 x + h7 y) + h8, u = (h0 x + h1 y) + h2,
               v = (h3 x + h4 y) + h5, du = X w - u, dv = Y w - v; inlier iff
               w > 0 and du du + dv dv <= (thr thr) (w w).
    best       highest count among the valid hypotheses, lowest index on ties.
               Fewer than 4 matches or no valid hypothesis: no model (h all 0,
               n_inliers 0, best_hypothesis -1, mask 0).
    refit      up to refit_rounds times.  Query and train are box-normalised
               over ALL the pair's matches (f64): centre (min + max) / 2 per
               axis, scale 2 / max(range_x, range_y, 1).  The 23 distinct sums
               of the 8 x 8 normal equations of the inhomogeneous system
               (h8 = 1) over the current inliers (SUMS), solved by Gaussian
               elimination with partial pivoting (_solve8); denormalised,
               divided by H[2][2], rounded to f32, rescored.  The round is
               accepted iff the nine values are finite and the count did not
               drop; stop at the first rejected round or when the mask did
               not change (that round still counts as accepted).

`variant` selects a deliberately wrong restatement (test use only): "tie_high"
highest index among equal counts, "thr_lt" a strict < in the inlier test,
"no_orient" no orientation check, "repeat" sampling with replacement.
"""
import numpy as np

VARIANTS = ("tie_high", "thr_lt", "no_orient", "repeat")
M32 = 0xFFFFFFFF


# ---- sampling ---------------------------------------------------------------
def mix32(x):
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def samples(seed, hyps, m, variant=None):
    """(len(hyps), 4) int64 indices into the pair's m >= 4 matches."""
    h = np.asarray(hyps, np.uint64)
    s = mix32(mix32((int(seed) + 0x9E3779B9) & M32) ^ h)
    picks = []
    for k in range(4):
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
def _area2(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def _adj(m):
    """Adjugate of 3 x 3 matrices given as m[r][c] (arrays); out[r][c]."""
    return [[m[1][1] * m[2][2] - m[1][2] * m[2][1], m[0][2] * m[2][1] - m[0][1] * m[2][2],
             m[0][1] * m[1][2] - m[0][2] * m[1][1]],
            [m[1][2] * m[2][0] - m[1][0] * m[2][2], m[0][0] * m[2][2] - m[0][2] * m[2][0],
             m[0][2] * m[1][0] - m[0][0] * m[1][2]],
            [m[1][0] * m[2][1] - m[1][1] * m[2][0], m[0][1] * m[2][0] - m[0][0] * m[2][1],
             m[0][0] * m[1][1] - m[0][1] * m[1][0]]]


def _basis(px, py):
    """px, py: (n, 4) f64.  The matrix sending the projective basis to the four points."""
    one = np.ones_like(px[:, 0])
    m = [[px[:, 0], px[:, 1], px[:, 2]], [py[:, 0], py[:, 1], py[:, 2]], [one, one, one]]
    a = _adj(m)
    lam = [(a[i][0] * px[:, 3] + a[i][1] * py[:, 3]) + a[i][2] for i in range(3)]
    return [[m[r][c] * lam[c] for c in range(3)] for r in range(3)]


def _mat3(b, a):
    return [[(b[r][0] * a[0][c] + b[r][1] * a[1][c]) + b[r][2] * a[2][c] for c in range(3)] for r in range(3)]


def models(rec, seed, hyps, variant=None):
    """H (n, 9) f32 and validity (n,) bool of hypotheses `hyps` on the records rec (m >= 4, 4) f32."""
    rec = np.asarray(rec, np.float32)
    idx = samples(seed, hyps, len(rec), variant)
    p = rec[idx].astype(np.float64)  # (n, 4 points, 4)
    x, y, X, Y = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    valid = np.ones(len(idx), bool)
    if variant != "no_orient":
        for a, b, c in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
            sq = _area2(x[:, a], y[:, a], x[:, b], y[:, b], x[:, c], y[:, c])
            st = _area2(X[:, a], Y[:, a], X[:, b], Y[:, b], X[:, c], Y[:, c])
            valid &= (sq != 0) & (st != 0) & ((sq > 0) == (st > 0))
    with np.errstate(all="ignore"):
        h = _mat3(_basis(X, Y), _adj(_basis(x, y)))
        h = np.stack([h[r][c] / h[2][2] for r in range(3) for c in range(3)], 1).astype(np.float32)
    valid &= np.isfinite(h).all(1)
    return h, valid


# ---- score ------------------------------------------------------------------
def inlier_mask(rec, h, thr, variant=None):
    """rec (m, 4) f32; h (9,) or (n, 9) f32 -> bool (m,) or (n, m)."""
    rec = np.asarray(rec, np.float32)
    h = np.asarray(h, np.float32)
    g = h.reshape(-1, 9)[:, :, None]
    x, y, X, Y = (rec[None, :, k] for k in range(4))
    thr = np.float32(thr)
    with np.errstate(all="ignore"):
        w = (g[:, 6] * x + g[:, 7] * y) + g[:, 8]
        u = (g[:, 0] * x + g[:, 1] * y) + g[:, 2]
        v = (g[:, 3] * x + g[:, 4] * y) + g[:, 5]
        du = X * w - u
        dv = Y * w - v
        e, lim = du * du + dv * dv, (thr * thr) * (w * w)
        ok = (w > 0) & ((e < lim) if variant == "thr_lt" else (e <= lim))
    assert w.dtype == np.float32 and e.dtype == np.float32
    return ok[0] if h.ndim == 1 else ok


# ---- refit ------------------------------------------------------------------
SUMS = ("n", "x", "y", "xx", "xy", "yy", "X", "Y", "Xx", "Xy", "Yx", "Yy", "Xxx", "Xxy", "Xyy", "Yxx", "Yxy", "Yyy",
        "Rx", "Ry", "Rxx", "Rxy", "Ryy")  # R = X X + Y Y; a product reads left to right: Xxy = (X x) y


def _box(a, b):
    """Centre and scale of the box normalisation of two f32 coordinate columns."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    ca, cb = (a.min() + a.max()) / 2.0, (b.min() + b.max()) / 2.0
    return ca, cb, 2.0 / max(a.max() - a.min(), b.max() - b.min(), 1.0)


def _terms(x, y, X, Y):
    """The 23 per-match terms of SUMS (normalised f64 coordinates)."""
    Xx, Xy, Yx, Yy = X * x, X * y, Y * x, Y * y
    R = X * X + Y * Y
    Rx, Ry = R * x, R * y
    return [np.ones_like(x), x, y, x * x, x * y, y * y, X, Y, Xx, Xy, Yx, Yy, Xx * x, Xx * y, Xy * y, Yx * x, Yx * y,
            Yy * y, Rx, Ry, Rx * x, Rx * y, Ry * y]


def _normal_equations(S):
    A = np.zeros((8, 8))
    for o in (0, 3):
        A[o:o + 3, o:o + 3] = [[S["xx"], S["xy"], S["x"]], [S["xy"], S["yy"], S["y"]], [S["x"], S["y"], S["n"]]]
    A[0:3, 6:8] = [[-S["Xxx"], -S["Xxy"]], [-S["Xxy"], -S["Xyy"]], [-S["Xx"], -S["Xy"]]]
    A[3:6, 6:8] = [[-S["Yxx"], -S["Yxy"]], [-S["Yxy"], -S["Yyy"]], [-S["Yx"], -S["Yy"]]]
    A[6:8, 0:6] = A[0:6, 6:8].T
    A[6:8, 6:8] = [[S["Rxx"], S["Rxy"]], [S["Rxy"], S["Ryy"]]]
    b = np.array([S["Xx"], S["Xy"], S["X"], S["Yx"], S["Yy"], S["Y"], -S["Rx"], -S["Ry"]])
    return A, b


def _solve8(A, b):
    """Gaussian elimination with partial pivoting (first largest |pivot|), then back substitution."""
    A, b = A.copy(), b.copy()
    with np.errstate(all="ignore"):
        for k in range(8):
            p = k
            for r in range(k + 1, 8):
                if abs(A[r, k]) > abs(A[p, k]):
                    p = r
            if p != k:
                A[[k, p]] = A[[p, k]]
                b[[k, p]] = b[[p, k]]
            for r in range(k + 1, 8):
                f = A[r, k] / A[k, k]
                for c in range(k + 1, 8):
                    A[r, c] = A[r, c] - f * A[k, c]
                b[r] = b[r] - f * b[k]
        g = np.zeros(8)
        for k in range(7, -1, -1):
            s = b[k]
            for c in range(k + 1, 8):
                s = s - A[k, c] * g[c]
            g[k] = s / A[k, k]
    return g


def refit(rec, mask, order=None):
    """One least-squares H (9,) f32 on the inliers `mask` (not rescored).  `order` permutes the summation."""
    rec = np.asarray(rec, np.float32)
    cx, cy, s = _box(rec[:, 0], rec[:, 1])
    CX, CY, S_ = _box(rec[:, 2], rec[:, 3])
    r = rec[np.asarray(mask, bool)].astype(np.float64)
    if order is not None:
        r = r[order]
    t = _terms((r[:, 0] - cx) * s, (r[:, 1] - cy) * s, (r[:, 2] - CX) * S_, (r[:, 3] - CY) * S_)
    sums = {}
    for name, v in zip(SUMS, t):
        acc = 0.0
        for e in v:  # sequential: the order is part of what `order` permutes
            acc = acc + e
        sums[name] = acc
    g = _solve8(*_normal_equations(sums))
    with np.errstate(all="ignore"):
        # H = T_t^-1 G T_q,  T_q = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]],  T_t^-1 = [[1/S, 0, CX], [0, 1/S, CY], [0, 0, 1]]
        G = [[g[0] * s, g[1] * s, g[2] - (g[0] * s * cx + g[1] * s * cy)],
             [g[3] * s, g[4] * s, g[5] - (g[3] * s * cx + g[4] * s * cy)],
             [g[6] * s, g[7] * s, 1.0 - (g[6] * s * cx + g[7] * s * cy)]]
        H = [[G[0][c] / S_ + CX * G[2][c] for c in range(3)], [G[1][c] / S_ + CY * G[2][c] for c in range(3)], G[2]]
        return np.array([H[r_][c] / H[2][2] for r_ in range(3) for c in range(3)], np.float64).astype(np.float32)


# ---- the whole rule ---------------------------------------------------------
def verify(rec, threshold=3.0, iterations=1024, seed=0, refit_rounds=2, variant=None, trace=None):
    """-> (H (3, 3) f32, mask (m,) bool, info dict n_matches / n_inliers / best_hypothesis / refits).
    `trace`, a list, receives every H (9,) a refit round scored, accepted or not."""
    rec = np.asarray(rec, np.float32).reshape(-1, 4)
    m = len(rec)
    none = (np.zeros((3, 3), np.float32), np.zeros(m, bool),
            dict(n_matches=m, n_inliers=0, best_hypothesis=-1, refits=0))
    if m < 4:
        return none
    best, best_n, best_h = -1, -1, None
    for h0 in range(0, iterations, 256):
        hyps = np.arange(h0, min(h0 + 256, iterations))
        h, valid = models(rec, seed, hyps, variant)
        cnt = inlier_mask(rec, h, threshold, variant).sum(1)
        for i in np.nonzero(valid)[0]:
            if cnt[i] > best_n or (variant == "tie_high" and cnt[i] == best_n):
                best, best_n, best_h = int(hyps[i]), int(cnt[i]), h[i]
    if best < 0:
        return none
    mask = inlier_mask(rec, best_h, threshold, variant)
    refits = 0
    for _ in range(refit_rounds):
        h2 = refit(rec, mask)
        if not np.isfinite(h2).all():
            break
        if trace is not None:
            trace.append(h2)
        mask2 = inlier_mask(rec, h2, threshold, variant)
        if mask2.sum() < mask.sum():
            break
        same = np.array_equal(mask, mask2)
        best_h, mask, refits = h2, mask2, refits + 1
        if same:
            break
    return best_h.reshape(3, 3).copy(), mask, dict(n_matches=m, n_inliers=int(mask.sum()), best_hypothesis=best,
                                                   refits=refits)


def records(kq, kt, matches):
    """(m, 4) f32 records of matches (query_idx, train_idx, ...) between keypoint arrays (n, >= 2)."""
    qi, ti = np.asarray(matches[0], np.int64), np.asarray(matches[1], np.int64)
    kq, kt = np.asarray(kq, np.float32), np.asarray(kt, np.float32)
    return np.concatenate([kq[qi, :2], kt[ti, :2]], 1).astype(np.float32).reshape(-1, 4)


def project(h, xy):
    """(n, 2) f64 projections of points xy by h (3, 3)."""
    p = np.concatenate([np.asarray(xy, np.float64), np.ones((len(xy), 1))], 1) @ np.asarray(h, np.float64).T
    return p[:, :2] / p[:, 2:3]


def residuals(rec, h):
    """f64 distances |H (x, y) - (X, Y)| in train pixels."""
    rec = np.asarray(rec, np.float64)
    return np.hypot(*(project(h, rec[:, :2]) - rec[:, 2:4]).T)


# ---- fixtures ---------------------------------------------------------------
H_MILD = np.array([[1.02, 0.03, 6.0], [-0.02, 0.98, -4.0], [2e-5, -1e-5, 1.0]])


def planted(m, inlier_share, seed, h=H_MILD):
    """m records: query points uniform in 640 x 480, a share of them mapped by
    h with +-0.5 px uniform noise (the planted inliers), the rest to
    uniform-random train points; returns (rec f32, planted mask).  Everything
    stays inside 640 x 480 (train points are clipped)."""
    rng = np.random.default_rng(seed)
    q = rng.uniform([20, 20], [620, 460], (m, 2))
    t = project(h, q) + rng.uniform(-0.5, 0.5, (m, 2))
    good = rng.random(m) < inlier_share
    t[~good] = rng.uniform([0, 0], [640, 480], (int((~good).sum()), 2))
    t = np.clip(t, 0, 640)
    return np.concatenate([q, t], 1).astype(np.float32), good


# (m, planted share, seed) of the fixtures the refit tests use, on the GPU too
# (threshold 2.0, 512 hypotheses, seed = the fixture's); 300 matches with 30 %
# inliers is the case the minimal-sample stage alone recovers worst
REFIT_CASES = [(300, 0.3, 0), (300, 0.3, 1), (300, 0.3, 2), (65, 0.6, 3), (1030, 0.5, 4)]

# match counts of the pairs of segments(): empty pairs at the front, in the
# middle and at the end, sizes around the 1024-record chunk and the 64-lane
# wave; SEG_TWICE is listed a second time at the end of the call
SEG_MATCHES = [0, 300, 5, 0, 1030, 64, 3, 200, 0]
SEG_TWICE = 1


def segments(seed=21):
    """One keypoint arena for SEG_MATCHES: pair p matches segment 2p (query)
    against segment 2p + 1 (train).  Every pair is planted with H_MILD (60 %
    inliers), so a read past a pair's records finds its neighbour's, which
    are inliers of the same H, and raises n_inliers.  Each segment holds its
    pair's points in a shuffled order plus three decoys, so the matches'
    indices matter.  -> (kps (n, 5) f32, offsets, pairs, matches per pair,
    records per pair)."""
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


def translation_exact(m=40, thr=2.0, seed=3):
    """Integer coordinates under the integer translation (+5, -3); match 0 is
    displaced by exactly (thr, 0).  Every step is exact in f64 and f32, so
    `<=` keeps match 0 under any hypothesis drawn from the others and `<`
    drops it."""
    rng = np.random.default_rng(seed)
    q = rng.permutation(64 * 48)[:m]
    q = np.stack([q % 64, q // 64], 1).astype(np.float64) * 4 + 8
    t = q + [5.0, -3.0]
    t[0, 0] += thr
    return np.concatenate([q, t], 1).astype(np.float32)


def square_swapped():
    """A square onto itself with two neighbouring corners swapped."""
    q = np.array([[100, 100], [300, 100], [300, 300], [100, 300]], np.float32)
    return np.concatenate([q, q[[1, 0, 2, 3]]], 1)


def four(seed=11):
    """m = 4 under H_MILD without noise: every valid hypothesis scores 4."""
    rng = np.random.default_rng(seed)
    q = np.array([[50, 60], [600, 40], [580, 430], [70, 400]], np.float64) + rng.uniform(-5, 5, (4, 2))
    return np.concatenate([q, project(H_MILD, q)], 1).astype(np.float32)


def collinear(m=30):
    """All query (and train) points on one line: no valid sample."""
    a = np.arange(m, dtype=np.float32)
    return np.stack([10 + 3 * a, 20 + 2 * a, 15 + 3 * a, 22 + 2 * a], 1)


def duplicates(m=30):
    """Every match the same point pair."""
    return np.tile(np.array([[100, 120, 110, 115]], np.float32), (m, 1))


def near_threshold(rec, h, thr, margin=1e-2):
    """Indices of the matches whose f64 residual under h lies within `margin` px of thr."""
    return np.nonzero(np.abs(residuals(rec, h) - thr) < margin)[0]


def near_threshold_any(rec, thr, iterations, seed, refit_rounds, margin=1e-2):
    """The same under the final H of verify(...) and under every H one of its
    refit rounds scored, accepted or rejected: empty means that every mask and
    every accept / reject decision has `margin` px to spare."""
    trace = []
    H, _, info = verify(rec, thr, iterations, seed, refit_rounds, trace=trace)
    hs = ([H] if info["best_hypothesis"] >= 0 else []) + [t.reshape(3, 3) for t in trace]
    return sorted({int(i) for h in hs for i in near_threshold(rec, h, thr, margin)})
