"""The frame-pair proposal's restatement (pairs_ref.py) on the CPU alone: that
an exact comparison against it catches each wrong rule, and that the bait
arena does what it claims, before a GPU pass over it is trusted."""
import numpy as np
import pytest

import match_ref
import pairs_ref as R


def _differs(variant):
    inp, kw = R.fixture(variant)
    if isinstance(inp, dict):
        return R.propose(inp["scores"], **kw) != R.propose(inp["scores"], variant=variant, **kw)
    pairs, sc = R.run(*inp, **kw)
    vpairs, vsc = R.run(*inp, variant=variant, **kw)
    return pairs != vpairs or not np.array_equal(sc, vsc)


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_fixture_catches_variant(variant):
    assert _differs(variant)


def test_subset_rule_by_hand():
    kps = np.zeros((7, 5), np.float32)
    kps[:, R.SIZE] = [2, 9, 2, 9, 2, 1, 50]
    S = R.subsets(kps, [0, 6, 6, 7], 3)
    assert [s.tolist() for s in S] == [[0, 1, 3], [], [6]]
    assert R.subsets(kps, [0, 6], 3, "sel_tie_high")[0].tolist() == [1, 3, 4]
    assert R.subsets(kps, [0, 6], 6)[0].tolist() == [0, 1, 2, 3, 4, 5] == R.subsets(kps, [0, 6], 128)[0].tolist()


def test_scores_are_match_ref_counts():
    desc, kps, offs = R.arena([40, 0, 33, 1], seed=11)
    S = R.subsets(kps, offs, 16)
    sc = R.score_matrix(desc, kps, offs, 16, 0.8)
    assert sc.dtype == np.uint32 and sc.shape == (4, 4) and not np.diag(sc).any()
    assert sc[0, 2] == len(match_ref.match(desc[S[0]], desc[S[2]], 0.8, cross_check=True)[0]) and sc[0, 2] > 0
    assert not sc[1].any() and not sc[:, 1].any()  # the empty segment
    assert not sc[:, 3].any()  # one train row: no second neighbour, every query rejected
    sym = R.score_matrix(desc, kps, offs, 16, 0.0)
    assert np.array_equal(sym, sym.T) and sym[0, 3] == 1


def test_proposal_rule_by_hand():
    inp, kw = R.fixture("keep_both")
    assert R.propose(inp["scores"], **kw) == [(0, 1), (0, 2), (0, 3)]
    assert R.propose(inp["scores"], variant="keep_both", **kw) == [(0, 1)]
    assert R.propose(inp["scores"], 8, 0) == [(0, 1), (0, 2), (0, 3)]
    assert R.propose(inp["scores"], 11, 0) == [(0, 1), (0, 2)]
    inp, kw = R.fixture("rank_tie_high")
    assert R.propose(inp["scores"], **kw) == [(0, 1), (1, 3), (2, 3)]


def test_hub_arena_separates_either_from_both():
    desc, kps, offs = R.hub_arena()
    pairs, sc = R.run(desc, kps, offs, 128, 0.8, 8, 1)
    assert pairs == [(0, 1), (0, 2), (0, 3)]
    assert R.run(desc, kps, offs, 128, 0.8, 8, 1, variant="keep_both")[0] == [(0, 1)]
    assert sc[0, 1] > sc[0, 2] > sc[0, 3] >= 8


@pytest.mark.parametrize("lens,h", [([300, 129, 64, 130], 128), ([40, 9, 0, 12, 30], 8)])
def test_bait_arena(lens, h):
    desc, kps, offs, baits = R.bait_arena(lens, h, seed=21)
    S = R.subsets(kps, offs, h)
    taken = set(np.concatenate(S).tolist())
    assert baits and not taken & set(baits)
    inside = [b for b in baits if offs[0] <= b < offs[-1]]
    assert len(inside) == sum(n > h for n in lens)
    want = R.score_matrix(desc, kps, offs, h, 0.8)
    # equal sizes straddle the cut of the longest segment: some rows of the cut's size are taken, some are not
    s = int(np.argmax(lens))
    size, cut = kps[offs[s]:offs[s + 1], R.SIZE], kps[S[s], R.SIZE].min()
    assert (size == cut).sum() > (kps[S[s], R.SIZE] == cut).sum() > 0
    for variant in ("sel_extra", "past_end"):
        got = R.score_matrix(desc, kps, offs, h, 0.8, variant)
        assert (got.astype(np.int64) - want).max() > 0, variant
    # the rows outside the arena's segments: selected by a read past either end
    lo = R.score_matrix(desc, kps, np.concatenate([[0], offs[1:]]), h, 0.8)
    hi = R.score_matrix(desc, kps, np.concatenate([offs[:-1], [len(desc)]]), h, 0.8)
    assert (lo.astype(np.int64) - want).max() > 0 and (hi.astype(np.int64) - want).max() > 0


def test_permuted_arena_permutes_scores():
    desc, kps, offs = R.arena([33, 0, 65, 20], seed=4)
    perm = [2, 0, 3, 1]
    sc = R.score_matrix(desc, kps, offs, 16, 0.8)
    got = R.score_matrix(*R.permuted(desc, kps, offs, perm), 16, 0.8)
    assert np.array_equal(got, sc[np.ix_(perm, perm)]) and sc.any()
