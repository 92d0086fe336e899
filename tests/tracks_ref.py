"""numpy restatement of the feature tracks (sift_mi_build_tracks_device) and
the inputs its tests share: this file DEFINES the result; the GPU path
(csrc/tracks.hip) and the host program (host_tracks_main.cpp) are held to it.

    node       arena row r in [offsets[0], offsets[n_segs]); keypoint i of
               segment s is row offsets[s] + i
    edge       for every match m of pair p, m in [pair_offsets[p],
               pair_offsets[p + 1]), with keep[m] != 0 (keep None: all):
               offsets[query_seg] + query_idx -- offsets[train_seg] + train_idx.
               Matches outside [pair_offsets[0], pair_offsets[n_pairs]) do not
               exist; duplicates and self edges change nothing
    label      the smallest row of the connected component
    conflict   two rows of the component lie in one segment
    track      a component of at least min_length (>= 2) rows that, with
               drop_conflicts, is not in conflict; numbered 0.. by ascending
               label; members by ascending row
    outputs    track_of (N,) i32 (-1: none), offsets (n_tracks + 1,) u32,
               obs (seg, idx, x, y) per member with the keypoints' bit
               patterns, conflict (n_tracks,) u8

The components come from repeated minimum propagation over the edges with
pointer jumping, until nothing changes.

`variant` selects a deliberately wrong restatement (test use only; FIXTURES
names the input each one is caught on):
"no_seg_base" rows without the segment base, "train_on_query" the train index
based on the query segment, "keep_ignored", "min_length_edges" min_length
counted in edges, "conflict_ends" conflict judged from the first and last
member only, "first_appearance" tracks ordered by first appearance in the
match list, "read_outside" the matches outside the pairs' range read too.
"""
import numpy as np

VARIANTS = ("no_seg_base", "train_on_query", "keep_ignored", "min_length_edges", "conflict_ends",
            "first_appearance", "read_outside")
MATCH = np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("distance", "<f4")])
OBS = np.dtype([("seg", "<u4"), ("idx", "<u4"), ("x", "<f4"), ("y", "<f4")])


def records(q, t):
    rec = np.zeros(len(q), MATCH)
    rec["query_idx"], rec["train_idx"] = q, t
    return rec


def edges(offsets, pairs, matches, pair_offsets, keep=None, variant=None):
    """The kept matches as two arrays of rows relative to offsets[0], in match order."""
    offs = np.asarray(offsets, np.int64)
    po = np.asarray(pair_offsets, np.int64)
    n = int(offs[-1] - offs[0])
    a, b = [], []
    for p, (qs, ts) in enumerate(pairs):
        lo, hi = int(po[p]), int(po[p + 1])
        if variant == "read_outside":
            lo = 0 if p == 0 else lo
            hi = len(matches) if p == len(pairs) - 1 else hi
        m = matches[lo:hi]
        if keep is not None and variant != "keep_ignored":
            m = m[np.asarray(keep[lo:hi]) != 0]
        qb, tb = offs[qs] - offs[0], offs[ts] - offs[0]
        if variant == "no_seg_base":
            qb = tb = 0
        if variant == "train_on_query":
            tb = qb
        a.append(np.minimum(qb + m["query_idx"].astype(np.int64), max(n - 1, 0)))
        b.append(np.minimum(tb + m["train_idx"].astype(np.int64), max(n - 1, 0)))
    if not a:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(a), np.concatenate(b)


def labels(n, a, b):
    """Per row the smallest row of its component."""
    lab = np.arange(n, dtype=np.int64)
    while True:
        new = lab.copy()
        np.minimum.at(new, a, lab[b])
        np.minimum.at(new, b, lab[a])
        new = new[new]  # a row's label is a row of its component: so is that row's label
        if np.array_equal(new, lab):
            return lab
        lab = new


def tracks(offsets, pairs, matches, pair_offsets, keep=None, min_length=2, drop_conflicts=False, kps=None,
           variant=None):
    """dict(track_of, offsets, obs, conflict).  kps: the (rows, 5) f32 keypoint
    arena (row offsets[0] + i is node i); None leaves obs' x, y zero."""
    assert min_length >= 2
    offs = np.asarray(offsets, np.int64)
    n = int(offs[-1] - offs[0])
    a, b = edges(offs, pairs, matches, pair_offsets, keep, variant)
    lab = labels(n, a, b)
    rows = np.argsort(lab, kind="stable")  # members by (label, row)
    sl = lab[rows]
    seg = np.searchsorted(offs - offs[0], rows, side="right") - 1  # the last segment starting at or before the row
    head = np.ones(n, bool)
    head[1:] = sl[1:] != sl[:-1]
    start = np.nonzero(head)[0]
    end = np.append(start[1:], n)
    size = end - start
    comp = np.cumsum(head) - 1  # component of each sorted position
    same = np.zeros(n, bool)
    same[1:] = ~head[1:] & (seg[1:] == seg[:-1])
    confl = np.zeros(len(start), bool)
    confl[comp[same]] = True
    if variant == "conflict_ends":
        confl = (size > 1) & (seg[start] == seg[end - 1])
    length = size
    if variant == "min_length_edges":
        length = np.bincount(np.searchsorted(sl[start], lab[a]), minlength=len(start))
    kept = length >= min_length
    if variant == "min_length_edges":
        kept &= size >= 2
    if drop_conflicts:
        kept &= ~confl
    order = np.nonzero(kept)[0]  # ascending label
    if variant == "first_appearance" and len(order):
        first = np.full(n, len(a) + 1, np.int64)
        np.minimum.at(first, lab[a], np.arange(len(a)))
        order = order[np.argsort(first[sl[start[order]]], kind="stable")]
    track_of = np.full(n, -1, np.int32)
    t_offs = np.zeros(len(order) + 1, np.uint32)
    t_offs[1:] = np.cumsum(size[order])
    obs = np.zeros(int(t_offs[-1]), OBS)
    for t, c in enumerate(order):
        r = rows[start[c]:end[c]]
        track_of[r] = t
        o = obs[t_offs[t]:t_offs[t + 1]]
        o["seg"], o["idx"] = seg[start[c]:end[c]], r - (offs[seg[start[c]:end[c]]] - offs[0])
        if kps is not None:
            xy = np.asarray(kps, np.float32).reshape(-1, 5)[offs[0] + r, :2]
            o["x"], o["y"] = xy[:, 0], xy[:, 1]
    conflict = confl[order].astype(np.uint8)
    return dict(track_of=track_of, offsets=t_offs, obs=obs, conflict=conflict)


def equal(a, b):
    """Every output array equal, x / y as bit patterns."""
    return (np.array_equal(a["track_of"], b["track_of"]) and np.array_equal(a["offsets"], b["offsets"])
            and np.array_equal(a["conflict"], b["conflict"]) and a["obs"].tobytes() == b["obs"].tobytes())


# ---- inputs ---------------------------------------------------------------------
def keypoints(n, seed=0):
    """(n, 5) f32 rows with distinct x, y (and a NaN and a -0.0 pattern: obs copies bits)."""
    rng = np.random.default_rng(1000 + seed)
    k = rng.random((n, 5), dtype=np.float32) * 1000
    if n > 2:
        k[1, 0], k[2, 1] = np.float32(np.nan), np.float32(-0.0)
    return k


def case(seg_lens, pairs, per_pair, keep=None, base=0, **kw):
    """An input dict: per_pair[p] = (query_idx list, train_idx list)."""
    offs = base + np.concatenate([[0], np.cumsum(seg_lens)]).astype(np.int64)
    po = np.zeros(len(pairs) + 1, np.int64)
    po[1:] = np.cumsum([len(q) for q, _ in per_pair])
    q = np.concatenate([np.asarray(q, np.int64) for q, _ in per_pair]) if per_pair else np.zeros(0, np.int64)
    t = np.concatenate([np.asarray(t, np.int64) for _, t in per_pair]) if per_pair else np.zeros(0, np.int64)
    d = dict(offsets=offs, pairs=[tuple(p) for p in pairs], matches=records(q, t), pair_offsets=po,
             keep=None if keep is None else np.asarray(keep, np.uint8))
    d.update(kw)
    return d


def run(c, variant=None, kps=None, **over):
    kw = dict(min_length=c.get("min_length", 2), drop_conflicts=c.get("drop_conflicts", False))
    kw.update(over)
    return tracks(c["offsets"], c["pairs"], c["matches"], c["pair_offsets"], c["keep"], kps=kps, variant=variant, **kw)


def permuted(c, seed=0):
    """The same input with its pairs and, within each pair, its matches shuffled."""
    rng = np.random.default_rng(seed)
    po = c["pair_offsets"]
    order = rng.permutation(len(c["pairs"]))
    idx = [po[p] + rng.permutation(int(po[p + 1] - po[p])) for p in order]
    npo = np.full(len(order) + 1, po[0], np.int64)
    npo[1:] += np.cumsum([len(i) for i in idx], dtype=np.int64)
    flat = np.concatenate(idx).astype(np.int64) if idx else np.zeros(0, np.int64)
    d = dict(c)
    lo, hi = int(po[0]), int(po[-1])
    m = c["matches"].copy()
    m[lo:hi] = c["matches"][flat]
    d["matches"] = m
    if c["keep"] is not None:
        k = c["keep"].copy()
        k[lo:hi] = c["keep"][flat]
        d["keep"] = k
    d["pairs"] = [c["pairs"][p] for p in order]
    d["pair_offsets"] = npo
    return d


def chain(n_segs, per_seg=1, reverse=False):
    """Keypoint i of segment s matched to keypoint i of segment s + 1."""
    pairs = [(s, s + 1) for s in range(n_segs - 1)]
    if reverse:
        pairs = pairs[::-1]
    i = np.arange(per_seg)
    return case([per_seg] * n_segs, pairs, [(i, i)] * len(pairs))


def star(n_spokes):
    """Every keypoint of segment 1 matched to keypoint 0 of segment 0: the
    centre is row 0, the smallest, so every link goes to a cell of its own."""
    return case([1, n_spokes], [(1, 0)], [(np.arange(n_spokes), np.zeros(n_spokes, np.int64))])


def hub(n_spokes):
    """Every keypoint of segment 0 matched to the one keypoint of segment 1:
    the hub is the LARGEST row, so it is the root every match tries to link
    first (one CAS target for all of them); the spokes come in descending
    order, so each later match finds a root above its spoke and tries to link
    that same root again: the losers of every race retry on the winner."""
    return case([n_spokes, 1], [(0, 1)], [(np.arange(n_spokes)[::-1], np.zeros(n_spokes, np.int64))])


def random_graph(seg_lens, n_pairs, density, seed, base=0, keep_share=None):
    """n_pairs random segment pairs (self pairs included), each with about
    density * min(segment sizes) random matches."""
    rng = np.random.default_rng(seed)
    live = [s for s, n in enumerate(seg_lens) if n]
    pairs, per = [], []
    for _ in range(n_pairs):
        qs, ts = (int(rng.choice(live)), int(rng.choice(live))) if live else (0, 0)
        k = int(density * min(seg_lens[qs], seg_lens[ts])) if live else 0
        pairs.append((qs, ts))
        per.append((rng.integers(0, max(seg_lens[qs], 1), k), rng.integers(0, max(seg_lens[ts], 1), k)))
    total = sum(len(q) for q, _ in per)
    keep = None if keep_share is None else (rng.random(total) < keep_share).astype(np.uint8)
    return case(seg_lens, pairs, per, keep, base)


def panning(n_frames, per_frame, seed, skip=2, wrong=0.02, lost=0.1):
    """A batch-like scene: world point w is keypoint (w - 3 f) of frame f where
    visible (the camera pans 3 points per frame), frames matched to the next
    and to the one `skip` further; `lost` of the matches missing, `wrong` of
    them pointing at a random keypoint; the keep mask drops half of the wrong."""
    rng = np.random.default_rng(seed)
    pairs = [(f, f + 1) for f in range(n_frames - 1)] + [(f, f + skip) for f in range(n_frames - skip)]
    per, keep = [], []
    for a, b in pairs:
        shift = 3 * (b - a)
        q = np.arange(shift, per_frame)
        t = q - shift
        ok = rng.random(len(q)) >= lost
        q, t = q[ok], t[ok].copy()
        bad = rng.random(len(q)) < wrong
        t[bad] = rng.integers(0, per_frame, int(bad.sum()))
        per.append((q, t))
        keep.append(~(bad & (rng.random(len(q)) < 0.5)))
    return case([per_frame] * n_frames, pairs, per, np.concatenate(keep).astype(np.uint8))


def with_bait(c, before=3, after=3):
    """Matches planted before pair_offsets[0] and after pair_offsets[n_pairs]
    (valid indices for the first / last pair) that would merge components if
    read: each joins keypoint 0 of the pair's query segment to the last of its
    train segment."""
    offs, pairs = c["offsets"], c["pairs"]
    d = dict(c)

    def bait(p, k):
        qs, ts = pairs[p]
        nq, nt = int(offs[qs + 1] - offs[qs]), int(offs[ts + 1] - offs[ts])
        return records(np.arange(k) % max(nq, 1), (nt - 1 - np.arange(k)) % max(nt, 1))
    d["matches"] = np.concatenate([bait(0, before), c["matches"], bait(len(pairs) - 1, after)])
    d["pair_offsets"] = c["pair_offsets"] + before
    if c["keep"] is not None:
        d["keep"] = np.concatenate([np.ones(before, np.uint8), c["keep"], np.ones(after, np.uint8)])
    return d


def _variant_fixtures():
    f = {}
    # two segments of 4; row 1 of segment 0 -- row 2 of segment 1.  Without the bases: rows 1 -- 2
    f["no_seg_base"] = case([4, 4], [(0, 1)], [([1], [2])])
    # segment 1 -- segment 2: the train row belongs to segment 2
    f["train_on_query"] = case([3, 3, 3], [(1, 2)], [([0], [1])])
    f["keep_ignored"] = case([2, 2, 2], [(0, 1), (1, 2)], [([0], [0]), ([0], [0])], keep=[1, 0])
    # one edge, two rows: a track of min_length 2
    f["min_length_edges"] = case([2, 2], [(0, 1)], [([0], [1])])
    # segments 0, 1, 1, 2 in one component: the conflict sits between its ends
    f["conflict_ends"] = case([1, 2, 1], [(0, 1), (0, 1), (1, 2)], [([0], [0]), ([0], [1]), ([1], [0])])
    # the component of the higher rows comes first in the match list
    f["first_appearance"] = case([2, 2], [(0, 1)], [([1, 0], [1, 0])])
    # (read_outside: with_bait of a two-component input; the bait would join them)
    f["read_outside"] = with_bait(case([2, 2], [(0, 1)], [([0, 1], [0, 1])]), 1, 1)
    return f


FIXTURES = _variant_fixtures()

# The segment-arena shape of match_ref.SEG_LENS: empty segments, an empty pair
# and offsets[0] != 0.
SEG_LENS = [0, 1, 127, 128, 129, 300, 64, 0]
