"""numpy restatement of the 2-nearest-neighbour matcher and the inputs its
tests share (test_match_ref_cpu.py pins it to the CPU oracle's matcher;
test_gpu_match_knn.py holds the GPU path against it).

    d^2        int64 |q|^2 + |t|^2 - 2 q.t (the exact integer)
    top two    stable argsort of d^2 * 2^32 + index: (distance, index) ascending,
               OpenCV's insertion rule (lowest index first among equals)
    distance   np.sqrt(np.float32(d^2))      (batchDistL2_8u32f)
    ratio      kept iff d1 < np.float32(r) * d2 in f32; a query whose train set
               has fewer than two rows has no second neighbour: rejected
    cross      kept iff the nearest train row's nearest query (lowest index
               among equals) is the query itself

`variant` selects a deliberately wrong restatement (test use only):
"tie_high" highest index among equal distances, "skip_equal" a second
neighbour that must be strictly farther than the first, "ratio_le" <= in the
ratio test, "ratio_d2" the ratio applied to d^2 instead of d.
"""
import numpy as np

VARIANTS = ("tie_high", "skip_equal", "ratio_le", "ratio_d2")


def d2_matrix(q, t):
    q = np.asarray(q, np.uint8).reshape(-1, 128).astype(np.int64)
    t = np.asarray(t, np.uint8).reshape(-1, 128).astype(np.int64)
    return (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2 * (q @ t.T)


def _top2(d2, variant=None):
    """Per row of d2: indices (n, 2) int32 (-1 absent) and d^2 (n, 2) int64 (-1 absent)."""
    n, m = d2.shape
    idx = np.full((n, 2), -1, np.int32)
    val = np.full((n, 2), -1, np.int64)
    if m == 0:
        return idx, val
    col = np.arange(m, dtype=np.int64)
    key = d2 * (1 << 32) + (m - 1 - col if variant == "tie_high" else col)[None, :]
    order = np.argsort(key, axis=1, kind="stable")
    idx[:, 0] = order[:, 0]
    val[:, 0] = d2[np.arange(n), order[:, 0]]
    if variant == "skip_equal":
        for i in range(n):
            later = [j for j in order[i, 1:] if d2[i, j] > val[i, 0]]
            if later:
                idx[i, 1], val[i, 1] = later[0], d2[i, later[0]]
    elif m > 1:
        idx[:, 1] = order[:, 1]
        val[:, 1] = d2[np.arange(n), order[:, 1]]
    return idx, val


def _dist(val):
    d = np.sqrt(np.maximum(val, 0).astype(np.float32))
    return np.where(val >= 0, d, np.float32(np.inf)).astype(np.float32)


def neighbors(q, t, variant=None):
    """knnMatch(q, t, 2): (idx (n, 2) int32, dist (n, 2) f32); -1 / inf where absent."""
    idx, val = _top2(d2_matrix(q, t), variant)
    return idx, _dist(val)


def match(q, t, ratio=0.0, cross_check=True, variant=None):
    """(query_idx, train_idx, distance) of the kept queries, in query order."""
    d2 = d2_matrix(q, t)
    n, m = d2.shape
    idx, val = _top2(d2, variant)
    dist = _dist(val)
    keep = idx[:, 0] >= 0
    if cross_check and m and n:
        back = _top2(d2.T, variant)[0][:, 0]  # per train row its nearest query
        keep &= back[np.maximum(idx[:, 0], 0)] == np.arange(n)
    if ratio:
        r = np.float32(ratio)
        has2 = idx[:, 1] >= 0
        if variant == "ratio_d2":
            ok = val[:, 0].astype(np.float32) < r * val[:, 1].astype(np.float32)
        elif variant == "ratio_le":
            ok = dist[:, 0] <= r * dist[:, 1]
        else:
            ok = dist[:, 0] < r * dist[:, 1]
        keep &= has2 & ok
    k = np.nonzero(keep)[0]
    return k.astype(np.int32), idx[k, 0].astype(np.int32), dist[k, 0].astype(np.float32)


def planted(nq, nt, seed):
    """Uniform random u8 rows; the first min(nq, nt) // 3 queries are distinct
    train rows plus noise in [-3, 3], clipped."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (nq, 128), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 128), dtype=np.uint8)
    k = min(nq, nt) // 3
    rows = rng.permutation(nt)[:k]
    noise = rng.integers(-3, 4, (k, 128))
    q[:k] = np.clip(t[rows].astype(np.int64) + noise, 0, 255).astype(np.uint8)
    return q, t


def triples():
    """50 rows, each three times in train (copies 50 apart); the queries are
    the rows in reverse order."""
    rng = np.random.default_rng(9)
    base = rng.integers(0, 200, (50, 128), dtype=np.uint8)
    return base[::-1].copy(), np.concatenate([base, base, base])


SEG_LENS = [0, 1, 127, 128, 129, 300, 64]
PAIRS = [(s, s + 1) for s in range(len(SEG_LENS) - 1)] + \
        [(3, 3), (5, 2), (2, 5), (0, 4), (4, 0), (0, 0), (5, 2)]  # empty segment on either side; (5, 2) twice


def segment_arena():
    """One arena of the segments.  Wherever two non-empty segments touch, the
    last rows of the one before equal the first rows of the one after (up to
    8 rows, never more than half of either segment unless it has one row):
    each segment is preceded and followed by copies of its own rows, so a row
    or column bound that lets a tile read past its segment finds a copy of an
    in-segment row: a second neighbour at the same distance, or for the
    self pair a distance-0 match, under an index outside the segment."""
    rng = np.random.default_rng(77)
    offs = np.concatenate([[0], np.cumsum(SEG_LENS)]).astype(np.int64)
    rows = rng.integers(0, 256, (int(offs[-1]), 128), dtype=np.uint8)
    # some true matches between consecutive segments: noisy copies, mid-segment
    for s in range(1, len(SEG_LENS) - 1):
        k = min(SEG_LENS[s], SEG_LENS[s + 1]) // 4
        a, b = offs[s] + SEG_LENS[s] // 3, offs[s + 1] + SEG_LENS[s + 1] // 3
        noise = rng.integers(-3, 4, (k, 128))
        rows[b:b + k] = np.clip(rows[a:a + k].astype(np.int64) + noise, 0, 255).astype(np.uint8)
    live = [s for s in range(len(SEG_LENS)) if SEG_LENS[s]]
    for s, n in zip(live, live[1:]):
        half = lambda L: 1 if L == 1 else L // 2
        k = min(8, half(SEG_LENS[s]), half(SEG_LENS[n]))
        rows[offs[n]:offs[n] + k] = rows[offs[s + 1] - k:offs[s + 1]]
    return rows, offs
