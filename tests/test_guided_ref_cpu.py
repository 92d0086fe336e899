"""Pins guided_ref.py, the numpy restatement of guided matching: the planted
scene has what its docstring says, every deliberately wrong variant differs
from the rule on its named fixture, the gate is the verification's own mask,
and the superset property holds on verified scenes.  No GPU."""
import numpy as np
import pytest

import epipolar_ref
import guided_ref
import match_ref
import verify_ref

SHAPES = [(1, 1), (5, 1), (1, 2), (37, 300), (128, 128), (129, 257), (300, 129)]


def _pairs(m):
    return set(zip(m[0].tolist(), m[1].tolist()))


@pytest.mark.parametrize("kind", guided_ref.KINDS)
@pytest.mark.parametrize("nq,nt", SHAPES)
def test_scene_is_what_it_says(nq, nt, kind):
    s = guided_ref.scene(nq, nt, nq * 7 + nt, kind)
    adm = guided_ref.admissible(s["kq"], s["kt"], s["g"], s["thr"], kind)
    assert adm.shape == (nq, nt) and adm.any()  # every shape holds an admissible pair
    assert adm[s["planted"]].all()
    assert not adm[s["decoy"]].any()
    assert adm[s["second"]].all()
    if min(nq, nt) >= 37:
        assert len(s["decoy"][0]) >= 4 and len(s["second"][0]) >= 4
        assert adm.mean() < 0.05  # a gate, not a formality
        # the decoy is the unguided nearest: an exact copy
        d2 = match_ref.d2_matrix(s["dq"], s["dt"])
        assert (d2[s["decoy"]] == 0).all()
        # rule: the decoyed queries match their planted row, and the ratio test keeps the lone candidates
        qi, ti, _ = guided_ref.run(s, ratio=0.8, cross_check=False)
        got = dict(zip(qi.tolist(), ti.tolist()))
        planted = dict(zip(s["planted"][0].tolist(), s["planted"][1].tolist()))
        n3 = len(s["decoy"][0])
        assert all(got.get(int(q)) == planted[int(q)] for q in s["decoy"][0])
        lone = [q for q in s["planted"][0][2 * n3:] if adm[q].sum() == 1]
        assert all(int(q) in got for q in lone)
        if kind == "homography":  # an F gate admits a whole band: few queries there have a single candidate
            assert len(lone) >= 4


@pytest.mark.parametrize("kind", guided_ref.KINDS)
def test_gate_is_the_verification_mask(kind):
    """admissible() on the records of a match set is the mask the verification computes for them."""
    mod = verify_ref if kind == "homography" else epipolar_ref
    rec, _ = mod.planted(200, 0.6, 3)
    g, mask, info = mod.verify(rec, threshold=2.0, iterations=256, seed=3)
    assert info["n_inliers"] > 50
    adm = guided_ref.admissible(rec[:, :2], rec[:, 2:4], g, 2.0, kind)
    assert np.array_equal(np.diag(adm), mask)
    assert not guided_ref.admissible(rec[:, :2], rec[:, 2:4], np.zeros(9), 2.0, kind).any()  # no model
    nan = np.full((1, 2), np.nan, np.float32)
    assert not guided_ref.admissible(nan, rec[:, 2:4], g, 2.0, kind).any()
    assert not guided_ref.admissible(rec[:, :2], nan, g, 2.0, kind).any()


@pytest.mark.parametrize("name", guided_ref.VARIANTS)
def test_variant_differs_on_its_fixture(name):
    f = guided_ref.variant_fixture(name)
    rule, wrong = guided_ref.run(f), guided_ref.run(f, variant=name)
    assert _pairs(rule) != _pairs(wrong), name
    assert len(rule[0]) > 0


def test_variant_fixtures_say_what_they_catch():
    f = guided_ref.variant_fixture("cross_ungated")
    assert _pairs(guided_ref.run(f)) == {(0, 0)} and not _pairs(guided_ref.run(f, variant="cross_ungated"))
    f = guided_ref.variant_fixture("gate_lt")
    assert _pairs(guided_ref.run(f)) == {(0, 0)} and not _pairs(guided_ref.run(f, variant="gate_lt"))
    f = guided_ref.variant_fixture("no_w_test")
    assert _pairs(guided_ref.run(f)) == {(1, 1)} and _pairs(guided_ref.run(f, variant="no_w_test")) == {(0, 0), (1, 1)}
    f = guided_ref.variant_fixture("tie_high")
    assert _pairs(guided_ref.run(f)) == {(0, 1)} and _pairs(guided_ref.run(f, variant="tie_high")) == {(0, 4)}


def test_ratio_and_cap():
    s = guided_ref.scene(129, 257, 11, "fundamental")
    base = guided_ref.run(s, cross_check=False)
    r = guided_ref.run(s, ratio=0.8, cross_check=False)
    assert 0 < len(r[0]) < len(base[0])  # unplanted queries with two random candidates in the band fail it
    cap = guided_ref.run(s, cross_check=False, max_distance=300.0)
    assert 0 < len(cap[0]) < len(base[0]) and cap[2].max() <= 300.0
    assert _pairs(cap) <= _pairs(base)
    # ratio 1.0 with two candidates at one distance: strict <, rejected
    f = guided_ref.variant_fixture("tie_high")
    assert not _pairs(guided_ref.run(f, ratio=1.0))


def test_empty_sides_and_zero_model():
    s = guided_ref.scene(37, 300, 5)
    e, ek = np.zeros((0, 128), np.uint8), np.zeros((0, 5), np.float32)
    assert len(guided_ref.match(e, s["dt"], ek, s["kt"], s["g"], 3.0)[0]) == 0
    assert len(guided_ref.match(s["dq"], e, s["kq"], ek, s["g"], 3.0)[0]) == 0
    assert len(guided_ref.match(s["dq"], s["dt"], s["kq"], s["kt"], np.zeros(9), 3.0)[0]) == 0


@pytest.mark.parametrize("m,share,seed", [(37, 0.6, 1), (128, 0.5, 2), (257, 0.4, 3), (300, 0.3, 0)])
def test_superset_of_verified_inliers(m, share, seed):
    dq, dt, kq, kt = guided_ref.verified_scene(m, share, seed)
    qi, ti, dist = match_ref.match(dq, dt, 0.0, True)
    assert len(qi) >= m - 2
    rec = verify_ref.records(kq, kt, (qi, ti))
    H, mask, info = verify_ref.verify(rec, threshold=2.0, iterations=256, seed=seed)
    assert info["n_inliers"] >= 8
    got = guided_ref.match(dq, dt, kq, kt, H, 2.0, "homography", 0.0, True)
    assert set(zip(qi[mask].tolist(), ti[mask].tolist())) <= _pairs(got)
    # and the distances of the shared matches are the unguided ones
    d = dict(zip(zip(got[0].tolist(), got[1].tolist()), got[2].tolist()))
    assert all(d[(a, b)] == c for a, b, c in zip(qi[mask].tolist(), ti[mask].tolist(), dist[mask].tolist()))
