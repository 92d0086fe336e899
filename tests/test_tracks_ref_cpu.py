"""The feature-track rule (tracks_ref.py) on the CPU: hand-worked results,
each named wrong variant told from the rule on its fixture, and the stated
properties (independence of the order of pairs and matches; no two members of
one segment under conflicts="drop")."""
import numpy as np
import pytest

import tracks_ref as T


def _plain_union_find(n, a, b):
    """The same components from a textbook union-find (smaller root wins)."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for x, y in zip(a.tolist(), b.tolist()):
        x, y = find(x), find(y)
        if x != y:
            parent[max(x, y)] = min(x, y)
    return np.array([find(x) for x in range(n)], np.int64)


def test_hand_worked_chain():
    c = T.chain(4, per_seg=2)  # rows 0..7; tracks {0, 2, 4, 6} and {1, 3, 5, 7}
    kps = T.keypoints(8)
    r = T.run(c, kps=kps)
    assert r["track_of"].tolist() == [0, 1, 0, 1, 0, 1, 0, 1]
    assert r["offsets"].tolist() == [0, 4, 8] and r["conflict"].tolist() == [0, 0]
    assert r["obs"]["seg"].tolist() == [0, 1, 2, 3, 0, 1, 2, 3]
    assert r["obs"]["idx"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert np.array_equal(r["obs"]["x"].view(np.uint32), kps[[0, 2, 4, 6, 1, 3, 5, 7], 0].view(np.uint32))
    assert np.array_equal(r["obs"]["y"].view(np.uint32), kps[[0, 2, 4, 6, 1, 3, 5, 7], 1].view(np.uint32))
    assert T.equal(T.run(T.chain(4, per_seg=2, reverse=True), kps=kps), r)


def test_hand_worked_star_and_min_length():
    c = T.star(5)  # row 0 and rows 1..5 of segment 1: one component, in conflict
    r = T.run(c)
    assert r["track_of"].tolist() == [0] * 6 and r["conflict"].tolist() == [1]
    d = T.run(c, drop_conflicts=True)
    assert d["track_of"].tolist() == [-1] * 6 and len(d["offsets"]) == 1 and len(d["obs"]) == 0
    assert T.run(c, min_length=6)["offsets"].tolist() == [0, 6]
    assert T.run(c, min_length=7)["offsets"].tolist() == [0]


def test_base_row_self_pairs_duplicates_and_self_edges():
    c = T.case([3, 2], [(0, 0), (0, 1), (0, 1)], [([1, 2], [1, 0]), ([0], [1]), ([0], [1])], base=40)
    r = T.run(c)  # rows: 1 -- 1 (nothing), 2 -- 0, 0 -- 4 twice: {0, 2, 4}
    assert r["track_of"].tolist() == [0, -1, 0, -1, 0] and r["conflict"].tolist() == [1]
    assert r["obs"]["seg"].tolist() == [0, 0, 1] and r["obs"]["idx"].tolist() == [0, 2, 1]
    kps = T.keypoints(45)
    assert np.array_equal(T.run(c, kps=kps)["obs"]["x"].view(np.uint32), kps[[40, 42, 44], 0].view(np.uint32))


@pytest.mark.parametrize("seed", range(4))
def test_labels_equal_a_plain_union_find(seed):
    c = T.random_graph([0, 5, 40, 17, 0, 64], 12, 0.4, seed, base=3 * seed, keep_share=0.7)
    a, b = T.edges(c["offsets"], c["pairs"], c["matches"], c["pair_offsets"], c["keep"])
    n = int(c["offsets"][-1] - c["offsets"][0])
    assert np.array_equal(T.labels(n, a, b), _plain_union_find(n, a, b))


@pytest.mark.parametrize("variant", T.VARIANTS)
def test_wrong_variants_are_caught(variant):
    c = T.FIXTURES[variant]
    assert not T.equal(T.run(c), T.run(c, variant=variant)), variant
    # the other fixtures' inputs are valid too: the rule runs on each
    assert len(T.run(c)["offsets"]) >= 1


def test_the_set_of_variants_is_the_documented_one():
    assert set(T.FIXTURES) == set(T.VARIANTS) and len(T.VARIANTS) == 7


def _inputs():
    return {
        "chain": T.chain(9, per_seg=3),
        "star": T.star(70),
        "hub": T.hub(70),
        "random": T.random_graph(T.SEG_LENS, 14, 0.3, 5, base=11, keep_share=0.8),
        "panning": T.panning(12, 60, 3),
        "bait": T.with_bait(T.random_graph([6, 7, 8], 5, 0.5, 2)),
    }


@pytest.mark.parametrize("name", sorted(_inputs()))
@pytest.mark.parametrize("drop", [False, True])
def test_order_of_pairs_and_matches_does_not_matter(name, drop):
    c = _inputs()[name]
    want = T.run(c, drop_conflicts=drop, min_length=3)
    for seed in range(3):
        assert T.equal(T.run(T.permuted(c, seed), drop_conflicts=drop, min_length=3), want)


@pytest.mark.parametrize("name", sorted(_inputs()))
def test_drop_leaves_no_two_members_of_one_segment(name):
    c = _inputs()[name]
    flag, drop = T.run(c), T.run(c, drop_conflicts=True)
    assert not drop["conflict"].any()
    for t in range(len(drop["offsets"]) - 1):
        seg = drop["obs"]["seg"][drop["offsets"][t]:drop["offsets"][t + 1]]
        assert len(np.unique(seg)) == len(seg) >= 2
    # the dropped tracks are exactly the flagged ones
    assert len(drop["offsets"]) - 1 == int((flag["conflict"] == 0).sum())
    for t in np.nonzero(flag["conflict"])[0]:
        seg = flag["obs"]["seg"][flag["offsets"][t]:flag["offsets"][t + 1]]
        assert len(np.unique(seg)) < len(seg)


def test_empty_inputs():
    for c in (T.case([5, 4], [], []), T.case([5, 4], [(0, 1), (1, 0)], [([], []), ([], [])]),
              T.case([5, 4], [(0, 1)], [([0, 1], [0, 1])], keep=[0, 0]), T.case([0, 0], [(0, 1)], [([], [])]),
              T.case([], [], [])):
        for cc in (c, T.permuted(c, 1)):
            r = T.run(cc)
            assert r["offsets"].tolist() == [0] and (r["track_of"] == -1).all() and len(r["obs"]) == 0


def test_panning_scene_has_long_tracks_and_some_conflicts():
    r = T.run(T.panning(12, 60, 3))
    length = np.diff(r["offsets"].astype(np.int64))
    assert length.max() >= 10 and 0 < r["conflict"].mean() < 0.5


def test_track_of_and_obs_agree():
    c = T.random_graph(T.SEG_LENS, 14, 0.3, 5, base=11)
    r = T.run(c)
    offs = c["offsets"] - c["offsets"][0]
    rows = offs[r["obs"]["seg"]] + r["obs"]["idx"]
    for t in range(len(r["offsets"]) - 1):
        m = rows[r["offsets"][t]:r["offsets"][t + 1]]
        assert (np.diff(m) > 0).all() and (r["track_of"][m] == t).all()
    assert (r["track_of"] >= 0).sum() == len(r["obs"])
    assert (np.diff(rows[r["offsets"][:-1]]) > 0).all()  # tracks by ascending label
