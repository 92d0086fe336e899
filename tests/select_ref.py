"""numpy restatement of the spread-limited selection (adaptive non-maximal
suppression; sift_mi_select_spread_device, csrc/select.hip) and the inputs its
tests share.  This text is the definition: the GPU equals it bit for bit.

The arena is kps[(N, 5) f32: x, y, size, angle, response] with offsets[n_segs
+ 1]; segments are independent.  Within one, for row i:

    suppressor  row j suppresses row i when r_i < c * r_j: f32 responses, one
                f32 multiply, strict.  0 < c <= 1.  Rows of equal response
                never suppress each other; a row never suppresses itself
                (responses are >= 0 and c * r rounds to at most r).
    radius      R2_i = min over suppressors j of
                (x_j - x_i) * (x_j - x_i) + (y_j - y_i) * (y_j - y_i), every
                operation a separately rounded f32 operation (numpy on f32
                arrays; no fused multiply-add); +inf without a suppressor
    selection   the min(n, limit) rows with the largest R2, compared as the
                u32 pattern of the f32 (numeric order for values >= 0 and
                +inf); the lower row first among equals; ascending rows

`variant` selects a deliberately wrong restatement (test use only):
  "le"                 <= in the suppressor test
  "c_wrong_side"       c * r_i < r_j
  "fused"              the squared distance as fma(dx, dx, dy * dy), evaluated
                       exactly (fractions.Fraction) and rounded once
  "tie_high"           among equal R2 the higher row first
  "rank_order"         the kept rows emitted by rank (R2 descending), not by row
  "stronger_or_equal"  a row j with c * r_j >= r_i suppresses, j == i included:
                       at c = 1 a row suppresses itself and its twins
  "arena_min"          the minimum runs over the whole arena, not the segment
"""
from fractions import Fraction

import numpy as np

VARIANTS = ("le", "c_wrong_side", "fused", "tie_high", "rank_order", "stronger_or_equal", "arena_min")
X, Y, RESPONSE = 0, 1, 4
CHUNK = 512  # query rows per numpy step: bounds the (rows, n) temporaries


def _round_f32(q):
    """The Fraction q >= 0 rounded once to f32, to nearest, ties to even."""
    a = np.float32(float(q))
    best = None
    for cand in (np.nextafter(a, np.float32(-np.inf)), a, np.nextafter(a, np.float32(np.inf))):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - q)
        even = (int(np.float32(cand).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[1]):
            best = (err, even, np.float32(cand))
    return best[2]


def _fused_dist2(dx, dy):
    """fma(dx, dx, dy * dy) elementwise: dy * dy rounded to f32, the sum with the exact dx * dx rounded once."""
    yy = (dy * dy).astype(np.float32)
    out = np.empty(dx.shape, np.float32)
    for idx in np.ndindex(dx.shape):
        out[idx] = _round_f32(Fraction(float(dx[idx])) * Fraction(float(dx[idx])) + Fraction(float(yy[idx])))
    return out


def radius2(kps, offsets, c, variant=None):
    """R2 (f32) of every row from offsets[0] to offsets[-1]."""
    kps = np.asarray(kps, np.float32).reshape(-1, 5)
    offs = np.asarray(offsets, np.int64)
    c = np.float32(c)
    out = np.full(int(offs[-1] - offs[0]), np.inf, np.float32)
    for s in range(len(offs) - 1):
        lo, hi = int(offs[s]), int(offs[s + 1])
        clo, chi = (int(offs[0]), int(offs[-1])) if variant == "arena_min" else (lo, hi)
        cx, cy, cr = kps[clo:chi, X], kps[clo:chi, Y], kps[clo:chi, RESPONSE]
        scaled = (c * cr).astype(np.float32)
        for q0 in range(lo, hi, CHUNK):
            q1 = min(q0 + CHUNK, hi)
            x, y, r = kps[q0:q1, X, None], kps[q0:q1, Y, None], kps[q0:q1, RESPONSE, None]
            if variant == "le":
                sup = r <= scaled[None, :]
                sup[np.arange(q1 - q0), np.arange(q0, q1) - clo] = False
            elif variant == "c_wrong_side":
                sup = (c * r).astype(np.float32) < cr[None, :]
            elif variant == "stronger_or_equal":
                sup = scaled[None, :] >= r
            else:
                sup = r < scaled[None, :]
            dx = (cx[None, :] - x).astype(np.float32)
            dy = (cy[None, :] - y).astype(np.float32)
            if variant == "fused":
                d = _fused_dist2(dx, dy)
            else:
                d = ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32)
            out[q0 - offs[0]:q1 - offs[0]] = np.where(sup, d, np.float32(np.inf)).min(axis=1, initial=np.inf)
    return out


def pick(r2, offsets, limit, variant=None):
    """(sel_offsets int64, rows uint32) from R2: per segment the min(n, limit)
    rows with the largest R2 pattern, the lower row first among equals, in
    ascending row order; rows are relative to their segment."""
    offs = np.asarray(offsets, np.int64)
    key = np.ascontiguousarray(r2, np.float32).view(np.uint32).astype(np.int64)
    sel, rows = [0], []
    for s in range(len(offs) - 1):
        lo, hi = int(offs[s] - offs[0]), int(offs[s + 1] - offs[0])
        idx = np.arange(hi - lo, dtype=np.int64)
        order = np.lexsort((-idx if variant == "tie_high" else idx, -key[lo:hi]))  # key descending, then the tie rule
        kept = order[:min(hi - lo, int(limit))]
        rows.append(kept if variant == "rank_order" else np.sort(kept))
        sel.append(sel[-1] + len(kept))
    return np.array(sel, np.int64), np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.uint32)


def run(kps, offsets, limit, c=0.9, variant=None):
    """(sel_offsets, rows, radius2) as a Selection holds them."""
    r2 = radius2(kps, offsets, c, variant)
    sel, rows = pick(r2, offsets, limit, variant)
    return sel, rows, r2


def arena_rows(offsets, sel_offsets, rows):
    """The kept rows as arena rows (int64): what the compact arena was gathered from."""
    offs, sel = np.asarray(offsets, np.int64), np.asarray(sel_offsets, np.int64)
    seg = np.repeat(np.arange(len(offs) - 1), np.diff(sel))
    return offs[seg] + np.asarray(rows, np.int64)


def occupied_cells(kps, width, height, grid=16):
    """How many cells of a grid x grid partition of the frame hold one of kps."""
    kps = np.asarray(kps, np.float32).reshape(-1, 5)
    gx = np.clip((kps[:, X].astype(np.float64) * grid / width).astype(np.int64), 0, grid - 1)
    gy = np.clip((kps[:, Y].astype(np.float64) * grid / height).astype(np.int64), 0, grid - 1)
    return len(set(zip(gx.tolist(), gy.tolist())))


def top_by_response(kps, limit):
    """What a features_limit keeps: the strongest responses, emission order among equals (ascending rows)."""
    kps = np.asarray(kps, np.float32).reshape(-1, 5)
    return np.sort(np.argsort(-kps[:, RESPONSE].astype(np.float64), kind="stable")[:limit])


# ---- inputs ---------------------------------------------------------------------
RESPONSES = np.array([0.01, 0.02, 0.02, 0.04, 0.05, 0.08], np.float32)  # few values: equal responses everywhere


def arena(seg_lens, seed, kind="grid", base=0, tail=0):
    """(kps, offsets): `base` rows before the first segment and `tail` after
    the last.  kind "grid": positions on an integer grid about sqrt(n) wide
    (every third row repeats the position of the row before it, as SIFT's
    orientation peaks do) and responses from RESPONSES but for one row of 1.0,
    so equal R2 and equal responses straddle every cut; kind "float": generic
    floats, the responses crowded towards 0 as SIFT's are."""
    rng = np.random.default_rng(seed)
    offs = base + np.concatenate([[0], np.cumsum(seg_lens)]).astype(np.int64)
    total = int(offs[-1]) + tail
    kps = (rng.random((total, 5), dtype=np.float32) * 100).astype(np.float32)
    if kind == "grid":
        for s, n in enumerate(seg_lens):
            if not n:
                continue
            side = max(2, int(np.sqrt(n)))
            k = kps[offs[s]:offs[s + 1]]
            k[:, X] = rng.integers(0, side, n).astype(np.float32)
            k[:, Y] = rng.integers(0, side, n).astype(np.float32)
            k[:, RESPONSE] = RESPONSES[rng.integers(0, len(RESPONSES), n)]
            twin = np.arange(2, n, 3)
            k[twin, :2] = k[twin - 1, :2]
            k[rng.integers(0, n), RESPONSE] = np.float32(1.0)  # one row above all: few infinite radii
    else:
        kps[:, X] = (rng.random(total, dtype=np.float32) * 1920).astype(np.float32)
        kps[:, Y] = (rng.random(total, dtype=np.float32) * 1080).astype(np.float32)
        u = rng.random(total, dtype=np.float32)
        kps[:, RESPONSE] = (u * u * u * u * np.float32(0.1)).astype(np.float32)  # few rows near the top
    return kps, offs


def bait_arena(seg_lens, seed, kind="float", base=3, tail=3):
    """arena() whose neighbours are baits: the first row of every non-empty
    segment and the `base` rows before offsets[0] and `tail` rows after
    offsets[-1] carry a huge response and sit exactly on a keypoint of the
    neighbouring segment (the last row of the one before, the first of the one
    after; the outer rows on the arena's first and last segment).  A lane that
    reads one row past a bound finds a suppressor at distance 0: a radius
    drops to 0 and `rows` changes.  Inside its own segment a huge first row is
    just a strong keypoint."""
    kps, offs = arena(seg_lens, seed, kind, base, tail)
    live = [s for s in range(len(seg_lens)) if seg_lens[s]]
    huge = np.float32(1e6)
    for a, b in zip(live, live[1:]):
        kps[offs[b], RESPONSE] = huge
        kps[offs[b], :2] = kps[offs[a + 1] - 1, :2]  # on the last row of the live segment before it
    first, last = live[0], live[-1]
    kps[offs[first], RESPONSE] = huge
    for row in range(base):
        kps[row, RESPONSE] = huge
        kps[row, :2] = kps[offs[first] + (1 + row) % seg_lens[first], :2]
    for i, row in enumerate(range(int(offs[-1]), int(offs[-1]) + tail)):
        kps[row, RESPONSE] = huge
        kps[row, :2] = kps[offs[last + 1] - 1 - i % seg_lens[last], :2]
    return kps, offs


def permuted(kps, offsets, perm):
    """The arena with its segments in the order perm (new segment i = old perm[i])."""
    offs = np.asarray(offsets, np.int64)
    rows = np.concatenate([np.arange(offs[p], offs[p + 1]) for p in perm]).astype(np.int64)
    lens = [int(offs[p + 1] - offs[p]) for p in perm]
    return kps[rows], np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _kps(rows):
    """(x, y, response) triples -> keypoints (size and angle 1)."""
    k = np.ones((len(rows), 5), np.float32)
    k[:, [X, Y, RESPONSE]] = np.array(rows, np.float32).reshape(-1, 3)
    return k


def fused_fixture():
    """Three rows.  Row 0 (response 10) suppresses rows 1 and 2 (response 1
    each: no test between them holds).  One of the two, B, lies at (dx, dy)
    from row 0 with dx * dx + dy * dy = p * p in separately rounded f32
    operations but not as fma(dx, dx, dy * dy); the other, C, at (p, 0), whose
    squared distance p * p is exact either way.  limit 2 keeps row 0 (inf) and
    one of the two: unfused they tie and the lower row is kept, fused B's
    radius is the smaller or the larger by one unit in the last place, and B
    is placed (row 1 or row 2) so that this keeps the other row."""
    rng = np.random.default_rng(2005)
    p = np.float32(1000.0)
    pp = np.float32(p * p)
    while True:
        dx = np.float32(rng.random() * 999.0 + 0.5)
        dy = np.float32(np.sqrt(np.float64(pp) - np.float64(dx) * np.float64(dx)))
        for _ in range(8):
            unfused = np.float32(np.float32(dx * dx) + np.float32(dy * dy))
            if unfused == pp:
                break
            dy = np.nextafter(dy, np.float32(0.0 if unfused > pp else np.inf))
        if unfused != pp:
            continue
        fused = _fused_dist2(np.array([dx]), np.array([dy]))[0]
        if fused != pp:
            break
    b, cc = (dx, dy, 1.0), (p, 0.0, 1.0)
    # fused below: B must be row 1 (kept by the tie unfused, cut when fused); fused above: row 2
    rows = [(0.0, 0.0, 10.0), b, cc] if fused < pp else [(0.0, 0.0, 10.0), cc, b]
    return _kps(rows), np.array([0, 3], np.int64)


def fixture(variant):
    """((kps, offsets), keyword arguments of run()) on which `variant` changes the result."""
    if variant == "le":  # r_1 == 0.5 * r_0 exactly: row 0 does not suppress row 1, only the far row 3 does
        k = _kps([(0, 0, 8.0), (1, 0, 4.0), (50, 0, 1.0), (100, 0, 16.0)])
        return (k, np.array([0, 4], np.int64)), dict(limit=3, c=0.5)
    if variant == "c_wrong_side":  # 10 vs 9.5 at c = 0.9: not a suppressor, but 0.9 * 9.5 < 10
        k = _kps([(0, 0, 10.0), (1, 0, 9.5), (40, 0, 5.0), (90, 0, 20.0)])
        return (k, np.array([0, 4], np.int64)), dict(limit=2, c=0.9)
    if variant == "fused":
        return fused_fixture(), dict(limit=2, c=0.9)
    if variant == "tie_high":  # rows 1, 2, 3 at distance 5 from row 0: row 1 is kept, not row 3
        k = _kps([(0, 0, 9.0), (5, 0, 1.0), (0, 5, 1.0), (3, 4, 1.0)])
        return (k, np.array([0, 4], np.int64)), dict(limit=2, c=0.9)
    if variant == "rank_order":  # the strongest row is the last one
        k = _kps([(0, 0, 1.0), (30, 0, 2.0), (70, 0, 9.0)])
        return (k, np.array([0, 3], np.int64)), dict(limit=3, c=0.9)
    if variant == "stronger_or_equal":  # two twins of equal response at one place, c = 1
        k = _kps([(0, 0, 5.0), (0, 0, 5.0), (10, 0, 7.0), (25, 0, 9.0)])
        return (k, np.array([0, 4], np.int64)), dict(limit=2, c=1.0)
    if variant == "arena_min":  # the next segment's strong first row sits on this segment's last row
        return bait_arena([5, 4, 6], 9, base=0, tail=0), dict(limit=3, c=0.9)
    raise KeyError(variant)
