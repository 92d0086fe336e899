"""numpy restatement of the frame-pair proposal (sift_mi_propose_pairs_device;
csrc/pairs.hip) and the inputs its tests share.  The matching rules (exact
integer d^2, lowest index among equals, cross check, f32 ratio test, a query
without a second neighbour rejected) are match_ref's and are not restated.

    subset    S_f = the min(n_f, h) rows of segment f with the largest `size`
              (keypoint column 2), compared as the u32 pattern of the f32,
              descending; the lower row first among equals; ascending rows
    score     score[a][b], a != b = len(match_ref.match(desc[S_a], desc[S_b],
              ratio, cross_check=True)); 0 on the diagonal
    proposal  s(a, b) = max(score[a][b], score[b][a]); a < b is a candidate
              when s >= min_matches; with max_partners > 0 each frame keeps
              its first max_partners candidates by (s descending, partner
              ascending) and a pair is proposed when either frame keeps it;
              sorted by (a, b)

`variant` selects a deliberately wrong restatement (test use only):
  "sel_tie_high"   among equal sizes the higher row first
  "sel_response"   selection by `response` (column 4) instead of `size`
  "sel_extra"      h + 1 rows are taken
  "past_end"       a segment's selection reads one row past its end
  "one_way"        the count has no cross check
  "ratio_le"       <= in the ratio test
  "lone_passes"    a query with no second neighbour passes the ratio test
                   (the guided matcher's rule)
  "s_min"          s(a, b) = min of the two directions
  "rank_tie_high"  among equal s the higher partner first
  "keep_both"      proposed only when both frames keep the pair
"""
import numpy as np

import match_ref

VARIANTS = ("sel_tie_high", "sel_response", "sel_extra", "past_end", "one_way", "ratio_le", "lone_passes", "s_min",
            "rank_tie_high", "keep_both")
SIZE, RESPONSE = 2, 4


def subsets(kps, offsets, h, variant=None):
    """Per segment the selected arena rows, ascending (int64)."""
    kps = np.asarray(kps, np.float32).reshape(-1, 5)
    offs = np.asarray(offsets, np.int64)
    col = RESPONSE if variant == "sel_response" else SIZE
    take = h + 1 if variant == "sel_extra" else h
    out = []
    for s in range(len(offs) - 1):
        end = int(offs[s + 1])
        if variant == "past_end":
            end = min(end + 1, len(kps))
        rows = np.arange(int(offs[s]), end, dtype=np.int64)
        key = np.ascontiguousarray(kps[rows, col]).view(np.uint32).astype(np.int64)
        tie = -rows if variant == "sel_tie_high" else rows
        order = np.lexsort((tie, -key))  # key descending, then the tie rule
        out.append(np.sort(rows[order[:take]]))
    return out


def score_matrix(desc, kps, offsets, h, ratio, variant=None):
    desc = np.asarray(desc, np.uint8).reshape(-1, 128)
    S = subsets(kps, offsets, h, variant)
    n = len(S)
    sc = np.zeros((n, n), np.uint32)
    mv = "ratio_le" if variant == "ratio_le" else None
    for a in range(n):
        for b in range(n):
            if a == b:
                continue
            r = ratio
            if variant == "lone_passes" and len(S[b]) < 2:
                r = 0.0
            sc[a, b] = len(match_ref.match(desc[S[a]], desc[S[b]], r, cross_check=variant != "one_way", variant=mv)[0])
    return sc


def propose(sc, min_matches, max_partners=0, variant=None):
    sc = np.asarray(sc).astype(np.int64)
    n = len(sc)
    s = np.minimum(sc, sc.T) if variant == "s_min" else np.maximum(sc, sc.T)
    cand = (s >= min_matches) & ~np.eye(n, dtype=bool)
    if max_partners == 0:
        keep = cand
    else:
        keep = np.zeros((n, n), bool)
        for f in range(n):
            p = np.nonzero(cand[f])[0]
            order = np.lexsort((-p if variant == "rank_tie_high" else p, -s[f, p]))
            keep[f, p[order[:max_partners]]] = True
    both = keep & keep.T if variant == "keep_both" else keep | keep.T
    return [(a, b) for a in range(n) for b in range(a + 1, n) if both[a, b]]


def run(desc, kps, offsets, h=128, ratio=0.8, min_matches=8, max_partners=0, variant=None):
    """(pairs, scores) as Context.propose_pairs_device returns them."""
    sc = score_matrix(desc, kps, offsets, h, ratio or 0.0, variant)
    return propose(sc, min_matches, max_partners, variant), sc


# ---- inputs ---------------------------------------------------------------------
SIZES = np.array([1.5, 2.0, 3.0, 4.0, 6.0, 8.0], np.float32)  # few values: equal sizes straddle every cut


def _noisy(rows, rng, amp=3):
    return np.clip(rows.astype(np.int64) + rng.integers(-amp, amp + 1, rows.shape), 0, 255).astype(np.uint8)


def arena(seg_lens, seed, base=0, tail=0):
    """(desc, kps, offsets): `base` rows before the first segment and `tail`
    rows after the last.  Between every two consecutive non-empty segments a
    third of the shorter one's rows are noisy copies (match_ref.planted's
    noise) of rows of the other, with sizes from the upper half of SIZES; each
    segment of >= 8 rows holds one row three times (distance ties: the lowest
    index wins) of which the next non-empty segment holds an exact copy
    (d1 = d2 = 0: the ratio test's < against <=); one all-0 and one all-255 row
    (the largest d^2) sit in the first two segments that have >= 4 rows."""
    rng = np.random.default_rng(seed)
    offs = base + np.concatenate([[0], np.cumsum(seg_lens)]).astype(np.int64)
    total = int(offs[-1]) + tail
    desc = rng.integers(0, 256, (total, 128), dtype=np.uint8)
    kps = (rng.random((total, 5), dtype=np.float32) * 100).astype(np.float32)
    kps[:, SIZE] = SIZES[rng.integers(0, len(SIZES), total)]
    live = [s for s in range(len(seg_lens)) if seg_lens[s]]
    for s, t in zip(live, live[1:]):
        k = min(seg_lens[s], seg_lens[t]) // 3
        ra = offs[s] + rng.permutation(seg_lens[s])[:k]
        rb = offs[t] + rng.permutation(seg_lens[t])[:k]
        desc[rb] = _noisy(desc[ra], rng)
        kps[ra, SIZE] = SIZES[rng.integers(3, len(SIZES), k)]
        kps[rb, SIZE] = SIZES[rng.integers(3, len(SIZES), k)]
        if seg_lens[s] >= 8 and seg_lens[t] >= 8:
            trip = offs[s] + rng.permutation(seg_lens[s])[:3]
            desc[trip] = desc[trip[0]]
            one = offs[t] + rng.integers(0, seg_lens[t])
            desc[one] = desc[trip[0]]
            kps[trip, SIZE] = SIZES[-1]
            kps[one, SIZE] = SIZES[-1]
    big = [s for s in live if seg_lens[s] >= 4][:2]
    for s, v in zip(big, (0, 255)):
        desc[offs[s] + 1] = v
        kps[offs[s] + 1, SIZE] = SIZES[-1]
    return desc, kps, offs


def bait_arena(seg_lens, h, seed, base=3, tail=3):
    """arena() with baits, (desc, kps, offsets, baits); baits = arena rows
    outside every S_f whose use raises a score:
      * in every segment f of more than h rows, the row ranked h + 1 by size
        is a byte copy of a row of some other S_g that no row of S_f matches
        and that matches no row of S_f (so taking h + 1 rows adds a match at
        distance 0);
      * the `base` rows before the first segment and the `tail` rows after the
        last carry huge sizes and such copies (a read past the arena's bounds
        selects them).
    The first row of every segment carries the largest of SIZES, so a selection
    that reads past the end of the segment before it takes that row (it is
    in its own segment's subset: a lure, not a bait)."""
    desc, kps, offs = arena(seg_lens, seed, base, tail)
    n = len(seg_lens)
    for s in range(n):
        if seg_lens[s]:
            kps[offs[s], SIZE] = SIZES[-1]
    S = subsets(kps, offs, h)
    ranked = subsets(kps, offs, h, "sel_extra")
    baits = []

    given = set()

    def lonely(f, g):
        """The rows of S_g outside every match between S_f and S_g that are no bait's source yet."""
        q, t, _ = match_ref.match(desc[S[f]], desc[S[g]], 0.0)
        q2, t2, _ = match_ref.match(desc[S[g]], desc[S[f]], 0.0)
        used = set(t.tolist()) | set(q2.tolist())
        rows = desc[S[g]]
        twice = [(rows == rows[i]).all(1).sum() > 1 for i in range(len(rows))]  # (a copy of these ties at d = 0)
        return [int(S[g][i]) for i in range(len(S[g])) if i not in used and not twice[i] and int(S[g][i]) not in given]

    def target(f):
        """A row of another subset for a bait of segment f: each bait gets its own."""
        for g in list(range(f + 1, n)) + list(range(f)):
            if len(S[g]) >= 2 and len(S[f]):
                free = lonely(f, g)
                if free:
                    given.add(free[0])
                    return free[0]
        return None

    for f in range(n):
        if seg_lens[f] > h:
            extra = np.setdiff1d(ranked[f], S[f])
            r = target(f)
            if len(extra) == 1 and r is not None:
                desc[extra[0]] = desc[r]
                baits.append(int(extra[0]))
    live = [s for s in range(n) if seg_lens[s]]
    outside = list(range(base)) + list(range(int(offs[-1]), int(offs[-1]) + tail))
    for i, row in enumerate(outside):
        f = live[0] if row < base else live[-1]
        r = target(f)
        if r is not None:
            desc[row] = desc[r]
        kps[row, SIZE] = np.float32(1e6)
        baits.append(row)
    return desc, kps, offs, baits


def hub_arena(seed=5):
    """Four frames: frame 0 holds three groups of 30, 20 and 10 rows, frames
    1, 2 and 3 a noisy copy of one group each (plus unrelated rows).  With
    max_partners = 1 frame 0 keeps only frame 1 while frames 2 and 3 keep
    frame 0: "either" proposes three pairs, "both" one."""
    rng = np.random.default_rng(seed)
    lens = [70, 40, 30, 20]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    desc = rng.integers(0, 256, (int(offs[-1]), 128), dtype=np.uint8)
    kps = (rng.random((int(offs[-1]), 5), dtype=np.float32) * 100).astype(np.float32)
    kps[:, SIZE] = SIZES[rng.integers(0, len(SIZES), len(kps))]
    start = 0
    for f, k in ((1, 30), (2, 20), (3, 10)):
        desc[offs[f]:offs[f] + k] = _noisy(desc[start:start + k], rng)
        start += k
    return desc, kps, offs


def permuted(desc, kps, offsets, perm):
    """The arena with its segments in the order perm (new segment i = old perm[i])."""
    offs = np.asarray(offsets, np.int64)
    rows = np.concatenate([np.arange(offs[p], offs[p + 1]) for p in perm]).astype(np.int64)
    lens = [int(offs[p + 1] - offs[p]) for p in perm]
    return desc[rows], kps[rows], np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


# ---- one fixture per wrong variant: (kind, input, parameters) --------------------
def _select_fixture(sizes, responses, h, seed):
    """Two segments: segment 0 with the given sizes / responses, segment 1 a
    noisy copy of exactly the rows of S_0 (and three unrelated rows)."""
    rng = np.random.default_rng(seed)
    n0 = len(sizes)
    kps0 = (rng.random((n0, 5), dtype=np.float32) * 100).astype(np.float32)
    kps0[:, SIZE], kps0[:, RESPONSE] = sizes, responses
    d0 = rng.integers(0, 256, (n0, 128), dtype=np.uint8)
    S0 = subsets(kps0, [0, n0], h)[0]
    d1 = np.concatenate([_noisy(d0[S0], rng), rng.integers(0, 256, (3, 128), dtype=np.uint8)])
    kps1 = np.ones((len(d1), 5), np.float32)
    return np.concatenate([d0, d1]), np.concatenate([kps0, kps1]), np.array([0, n0, n0 + len(d1)], np.int64)


def fixture(variant):
    """(arena or score matrix, keyword arguments) on which `variant` differs
    from the rule: an arena (desc, kps, offsets) for run(), or for the three
    proposal variants {"scores": matrix} for propose()."""
    if variant == "sel_tie_high":  # rows 1, 2, 3 tie at the cut: row 1 is taken, not row 3
        return _select_fixture([5, 3, 3, 3], [1, 1, 1, 1], 2, 1), dict(h=2, ratio=0.8, min_matches=1)
    if variant == "sel_response":  # the largest responses sit on the smallest sizes
        return _select_fixture([5, 4, 3, 2], [1, 2, 3, 4], 2, 2), dict(h=2, ratio=0.8, min_matches=1)
    if variant == "sel_extra":
        d, k, o, _ = bait_arena([6, 5], 4, 3, base=0, tail=0)
        return (d, k, o), dict(h=4, ratio=0.8, min_matches=1)
    if variant == "past_end":
        d, k, o, _ = bait_arena([6, 7, 5], 4, 4, base=0, tail=0)
        return (d, k, o), dict(h=4, ratio=0.8, min_matches=1)
    if variant == "one_way":  # two queries share their nearest train row: one of them is not mutual
        rng = np.random.default_rng(6)
        t = rng.integers(0, 256, (3, 128), dtype=np.uint8)
        q = np.concatenate([_noisy(t[:1], rng, 1), _noisy(t[:1], rng, 5)])
        kps = np.ones((5, 5), np.float32)
        return (np.concatenate([q, t]), kps, np.array([0, 2, 5], np.int64)), dict(h=4, ratio=0.0, min_matches=1)
    if variant == "ratio_le":  # the train set holds the query twice: d1 = d2 = 0
        rng = np.random.default_rng(7)
        q = rng.integers(0, 256, (1, 128), dtype=np.uint8)
        kps = np.ones((3, 5), np.float32)
        return (np.concatenate([q, q, q]), kps, np.array([0, 1, 3], np.int64)), dict(h=4, ratio=1.0, min_matches=1)
    if variant == "lone_passes":  # one train row: no second neighbour
        rng = np.random.default_rng(8)
        q = rng.integers(0, 256, (2, 128), dtype=np.uint8)
        kps = np.ones((3, 5), np.float32)
        return (np.concatenate([q, _noisy(q[:1], rng)]), kps, np.array([0, 2, 3], np.int64)), \
            dict(h=4, ratio=0.8, min_matches=1)
    if variant == "s_min":
        return {"scores": np.array([[0, 9], [3, 0]], np.uint32)}, dict(min_matches=8)
    if variant == "rank_tie_high":
        sc = np.zeros((4, 4), np.uint32)
        sc[0, 1] = sc[0, 2] = 10
        sc[1, 3] = sc[2, 3] = 20
        return {"scores": sc}, dict(min_matches=8, max_partners=1)
    if variant == "keep_both":
        sc = np.zeros((4, 4), np.uint32)
        sc[0, 1], sc[0, 2], sc[0, 3] = 30, 20, 10
        return {"scores": sc}, dict(min_matches=8, max_partners=1)
    raise KeyError(variant)
