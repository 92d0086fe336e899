"""The numpy restatement of the matcher (match_ref.py) against the CPU
oracle's BFMatcher restatement, and its teeth: every deliberately wrong
variant is caught by at least one of the shared fixtures.  No GPU."""
import numpy as np
import pytest

import match_ref

SHAPES = [(1, 1), (5, 1), (1, 2), (37, 300), (128, 128), (129, 257), (300, 129)]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and \
        np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


def _fixtures():
    out = [("triples",) + match_ref.triples()]
    for nq, nt in SHAPES:
        out.append((f"planted{nq}x{nt}",) + match_ref.planted(nq, nt, nq * 7 + nt))
    return out


@pytest.mark.parametrize("cross", [True, False])
def test_ratio_off_equals_oracle(oracle, cross):
    for name, q, t in _fixtures():
        got = match_ref.match(q, t, 0.0, cross)
        want = oracle.match(q, t, cross_check=cross)
        assert _same(got, want), name
        assert _same(match_ref.match(t, q, 0.0, cross), oracle.match(t, q, cross_check=cross)), name


def test_neighbors_are_ordered_and_first_is_the_match():
    for name, q, t in _fixtures():
        idx, dist = match_ref.neighbors(q, t)
        qi, ti, d = match_ref.match(q, t, 0.0, False)
        assert np.array_equal(idx[qi, 0], ti) and np.array_equal(dist[qi, 0], d), name
        if t.shape[0] > 1:
            assert np.all(dist[:, 0] <= dist[:, 1]) and np.all(idx[:, 0] != idx[:, 1]), name
        else:
            assert np.all(idx[:, 1] == -1) and np.all(np.isinf(dist[:, 1])), name
            assert len(match_ref.match(q, t, 1.0, False)[0]) == 0, name  # no second neighbour: rejected


def test_triples_second_is_the_second_copy():
    q, t = match_ref.triples()
    idx, dist = match_ref.neighbors(q, t)
    assert np.array_equal(idx[:, 0], np.arange(50)[::-1]) and np.array_equal(idx[:, 1], idx[:, 0] + 50)
    assert np.all(dist == 0)
    assert len(match_ref.match(q, t, 1.0, False)[0]) == 0  # 0 < 1.0 * 0 is false: strict


def test_planted_ratio_splits_the_queries():
    """At 0.8 the ratio test alone keeps the planted queries and rejects the
    rest: at least a quarter of min(nq, nt) kept (the planted third) and a
    quarter of the queries rejected; at 0.95 a few unplanted ones pass too."""
    for nq, nt in SHAPES[3:]:
        q, t = match_ref.planted(nq, nt, nq * 7 + nt)
        kept = len(match_ref.match(q, t, 0.8, False)[0])
        assert kept == min(nq, nt) // 3, (nq, nt, kept)
        assert 4 * kept >= min(nq, nt) and 4 * (nq - kept) >= nq, (nq, nt, kept)
        idx, dist = match_ref.neighbors(q, t)
        r = dist[:, 0] / dist[:, 1]
        assert r[:kept].max() < 0.1 and r[kept:].min() > 0.85, (nq, nt)
    borderline = sum(len(match_ref.match(*match_ref.planted(nq, nt, nq * 7 + nt), 0.95, False)[0])
                     - min(nq, nt) // 3 for nq, nt in SHAPES[3:])
    assert borderline > 0


@pytest.mark.parametrize("variant", match_ref.VARIANTS)
def test_wrong_variants_are_caught(variant):
    caught = []
    for name, q, t in _fixtures():
        for ratio in (0.0, 0.8, 0.95, 1.0):
            for cross in (True, False):
                if not _same(match_ref.match(q, t, ratio, cross), match_ref.match(q, t, ratio, cross, variant)):
                    caught.append((name, ratio, cross))
        a, b = match_ref.neighbors(q, t), match_ref.neighbors(q, t, variant)
        if not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])):
            caught.append((name, "neighbors"))
    assert caught, variant


def test_segment_arena_catches_bleed():
    """A matcher that takes rows past the end of a segment (a tile bound taken
    from the arena instead of the segment) differs from the reference on the
    segment fixture: on the train side and on the query side."""
    rows, offs = match_ref.segment_arena()
    assert [int(offs[s + 1] - offs[s]) for s in range(len(match_ref.SEG_LENS))] == match_ref.SEG_LENS
    seg = lambda s, extra=0: rows[offs[s]:min(offs[s + 1] + extra, len(rows))]
    train_caught, query_caught = [], []
    for a, b in match_ref.PAIRS:
        if not (match_ref.SEG_LENS[a] and match_ref.SEG_LENS[b]):
            continue
        for ratio in (0.0, 0.8, 1.0):
            want = match_ref.match(seg(a), seg(b), ratio, True)
            if not _same(want, match_ref.match(seg(a), seg(b, 16), ratio, True)):
                train_caught.append((a, b, ratio))
            got = match_ref.match(seg(a, 16), seg(b), ratio, True)
            keep = got[0] < len(seg(a))
            if not _same(want, tuple(x[keep] for x in got)):
                query_caught.append((a, b, ratio))
    # every pair with more than one query (segment 1 has a single row) and rows after its train segment
    last = len(match_ref.SEG_LENS) - 1
    many = {(a, b) for a, b in match_ref.PAIRS if match_ref.SEG_LENS[a] > 1 and match_ref.SEG_LENS[b] and b != last}
    assert {(a, b) for a, b, _ in train_caught} >= many, (many, train_caught)
    assert query_caught
