"""The spread-limited selection's restatement (select_ref.py) on the CPU alone:
that an exact comparison against it catches each wrong rule, that the bait
arena does what it claims, and that on the oracle's keypoints the selection
does what it is for (more of the frame covered than by the strongest
responses), before a GPU pass over it is trusted."""
import numpy as np
import pytest
from conftest import load_golden

import select_ref as R


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_fixture_catches_variant(variant):
    inp, kw = R.fixture(variant)
    want, got = R.run(*inp, **kw), R.run(*inp, variant=variant, **kw)
    assert not np.array_equal(want[1], got[1]), "the kept rows must change, not only a radius"


def test_rule_by_hand():
    k = R._kps([(0, 0, 8.0), (1, 0, 4.0), (50, 0, 1.0), (100, 0, 16.0), (7, 7, 3.0)])
    sel, rows, r2 = R.run(k, [0, 4, 4, 5], 3, c=0.5)
    # 8 < 0.5 * 16 is false: row 0 has no suppressor; the last segment's single row has none either
    assert r2.tolist() == [np.inf, 99.0 ** 2, 49.0 ** 2, np.inf, np.inf]
    assert sel.tolist() == [0, 3, 3, 4] and rows.tolist() == [0, 1, 3, 0] and rows.dtype == np.uint32
    assert R.arena_rows([0, 4, 4, 5], sel, rows).tolist() == [0, 1, 3, 4]
    assert R.run(k, [0, 4, 4, 5], 2 ** 31 - 1, c=0.5)[1].tolist() == [0, 1, 2, 3, 0]
    # c = 1: equal responses never suppress each other
    twins = R._kps([(0, 0, 5.0), (0, 0, 5.0), (3, 4, 6.0)])
    assert R.radius2(twins, [0, 3], 1.0).tolist() == [25.0, 25.0, np.inf]


def test_fused_fixture_differs_by_one_ulp_and_moves_the_cut():
    k, offs = R.fused_fixture()
    want, fused = R.radius2(k, offs, 0.9), R.radius2(k, offs, 0.9, "fused")
    assert want[1] == want[2] == np.float32(1e6) and np.isinf(want[0])
    b = int(np.argmax(fused != want))
    assert abs(int(fused[b].view(np.uint32)) - int(want[b].view(np.uint32))) == 1
    assert R.pick(want, offs, 2)[1].tolist() == [0, 1] and R.pick(fused, offs, 2)[1].tolist() == [0, 2]


def test_round_f32_is_one_rounding():
    from fractions import Fraction
    one, ulp = Fraction(1), Fraction(1, 2 ** 23)
    assert R._round_f32(one + ulp / 2) == np.float32(1.0)  # a tie: to even
    assert R._round_f32(one + ulp / 2 + Fraction(1, 2 ** 80)) == np.nextafter(np.float32(1), np.float32(2))
    assert R._round_f32(one + 3 * ulp / 2) == np.float32(1) + np.float32(2.0 ** -22)  # a tie: to even, upwards


@pytest.mark.parametrize("kind", ["grid", "float"])
def test_bait_arena(kind):
    lens = [40, 1, 0, 33, 2, 70]
    kps, offs = R.bait_arena(lens, 5, kind)
    want = R.run(kps, offs, 8)
    assert not _same(want, R.run(kps, offs, 8, variant="arena_min"))
    # a read past either end of the arena's segments, and past every inner bound
    lo = R.run(kps, np.concatenate([[0], offs[1:]]), 8)
    hi = R.run(kps, np.concatenate([offs[:-1], [len(kps)]]), 8)
    assert not np.array_equal(lo[1][:8], want[1][:8]) and not np.array_equal(hi[1][-8:], want[1][-8:])
    for s in range(len(lens) - 1):
        if lens[s] > 8:
            o2 = offs.copy()
            o2[s + 1] += 1  # segment s reads one row of its neighbour
            got = R.run(kps, o2, 8)
            assert not np.array_equal(got[1][want[0][s]:want[0][s + 1]], want[1][want[0][s]:want[0][s + 1]]), s


def test_grid_arena_has_ties_across_the_cut():
    kps, offs = R.arena([300], 3, "grid")
    sel, rows, r2 = R.run(kps, offs, 64)
    cut = r2[rows].min()
    assert (r2 == cut).sum() > (r2[rows] == cut).sum() > 0  # some rows of the cut's radius are kept, some are not
    assert len(np.unique(kps[:, R.RESPONSE])) <= len(R.RESPONSES)


def test_permuted_arena_permutes_selection():
    kps, offs = R.arena([33, 0, 65, 20], 4, "float")
    perm = [2, 0, 3, 1]
    sel, rows, r2 = R.run(kps, offs, 16)
    k2, o2 = R.permuted(kps, offs, perm)
    sel2, rows2, r22 = R.run(k2, o2, 16)
    for i, p in enumerate(perm):
        assert np.array_equal(rows2[sel2[i]:sel2[i + 1]], rows[sel[p]:sel[p + 1]])
        assert np.array_equal(r22[o2[i]:o2[i + 1]], r2[offs[p]:offs[p + 1]])


@pytest.mark.parametrize("name,n", [("bird_small", 100), ("tree_small", 200)])
def test_selection_covers_more_of_the_frame_than_top_responses(oracle, name, n):
    """OpenCV profile, c = 0.9, a 16 x 16 grid of cells over the frame."""
    img = load_golden(name)["image"]
    h, w = img.shape
    kps, _ = oracle.sift(img)
    sel, rows, r2 = R.run(kps, [0, len(kps)], n, c=0.9)
    spread = R.occupied_cells(kps[rows], w, h)
    strongest = R.occupied_cells(kps[R.top_by_response(kps, n)], w, h)
    print(name, n, "occupied cells: ANMS", spread, "top-N by response", strongest, "inf radii", int(np.isinf(r2).sum()))
    assert len(rows) == n and spread > strongest
    assert np.isinf(r2).sum() >= 1
