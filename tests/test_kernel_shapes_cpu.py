"""The threshold-shape table (tests/kernel_shapes.py) on the CPU alone: that
it says what it claims, before a GPU pass over it is trusted.

  * the mirror's octave count is the oracle's, and the table's literal tail
    octaves and launch counts are the mirror's;
  * every capacity case fills the tail kernel's LDS to within 16 floats, and
    its one-pixel-wider partner starts the tail at a later octave;
  * the cases of every predicate sit on both of its sides, at the values the
    table states;
  * the keypoint inputs give enough keypoints (>= 50 on frames of >= 3000
    pixels, >= 1 on smaller ones), and every seam case has an initial
    extremum within one column of its seam.  These two are conditions on the
    oracle's result alone: if one fails, the shape or the generator has to
    change, not the bound.
"""
import numpy as np
import pytest

import kernel_shapes as K

_memo = {}


def _oracle(oracle, case, profile):
    """{image name: (keypoints, descriptors, internal)} of the case's pattern
    images: computed once per (case, profile)."""
    key = (case.name, profile)
    if key not in _memo:
        _memo[key] = {n: oracle.sift(im, profile=profile, internal=True) for n, im in K.pattern_images(case).items()}
    return _memo[key]


def _ids(cases):
    return [c.name for c in cases]


def test_names_unique_and_documented():
    assert len(K.BY_NAME) == len(K.CASES)
    for c in K.CASES:
        assert ":" in c.target and c.why and c.opts in K.OPTION_SETS and all(a in K.OPTION_SETS for a in c.also), c.name
        assert c.w * c.h <= 32000, c.name  # small frames: the whole table runs in seconds


@pytest.mark.parametrize("case", K.CASES, ids=_ids(K.CASES))
def test_octaves_and_literals(oracle, case):
    sizes = K.octave_sizes(case.w, case.h)
    assert len(sizes) == oracle.n_octaves(case.w, case.h)
    py = oracle.Pyramid(K.noise(case.w, case.h))
    assert [py.dims(o) for o in range(py.n_octaves)] == sizes
    for p in K.PROFILES:
        assert (case.tail[p], case.launches[p]) == K.dispatch(case.w, case.h, p, K.OPTION_SETS[case.opts]), p


def test_issue_launch_counts():
    """The OpenCV default counts derived by hand from PyramidRun: seed pair + 3
    + tail; seed + (1, 2) pair octave + tail; seed + five single blurs + tail."""
    want = {"seed_80x40": 5, "seed_79x40": 6, "seed_80x32": 5, "seed_80x31": 7}
    assert {n: K.BY_NAME[n].launches[K.OPENCV] for n in want} == want
    # the frame sizes of the benchmark and the parity suite: tail from octave 5 / 4
    assert K.dispatch(1920, 1080, K.OPENCV) == (5, 21) and K.dispatch(640, 480, K.OPENCV) == (4, 17)


CAPACITY = [c for c in K.CASES if c.kind == "capacity"]


@pytest.mark.parametrize("case", CAPACITY, ids=_ids(CAPACITY))
def test_capacity(case):
    p = case.cap
    sizes = K.octave_sizes(case.w, case.h)
    o = K.tail_octave_start(sizes, p)
    assert o == case.tail[p] and o < len(sizes)
    use = K.tail_use(*sizes[o], p)
    assert K.K_TAIL_LDS_FLOATS - 16 <= use <= K.K_TAIL_LDS_FLOATS, use
    partners = [c for c in K.CASES if c.partner == case.name]
    if not partners:  # the wider frame is itself a capacity case
        assert f"{case.w + 1}x{case.h}" in K.CAPACITY[p]
        return
    (q,) = partners
    assert (q.w, q.h) == (case.w + 1, case.h)
    qs = K.octave_sizes(q.w, q.h)
    assert K.tail_use(*qs[o], p) > K.K_TAIL_LDS_FLOATS
    assert K.tail_octave_start(qs, p) > o and q.tail[p] > case.tail[p]
    # the other profile, where the same octave stays under the limit
    other = 1 - p
    if K.tail_octave_start(sizes, other) == o:
        assert K.tail_use(*sizes[o], other) <= K.K_TAIL_LDS_FLOATS


PREDICATED = [c for c in K.CASES if c.pred]


@pytest.mark.parametrize("case", PREDICATED, ids=_ids(PREDICATED))
def test_predicate_value(case):
    for p in K.PROFILES:
        if case.holds[p] is not None:
            assert K.predicate(case, p) is case.holds[p], p


def test_predicate_groups_have_both_sides():
    groups = {}
    for c in PREDICATED:
        for p in K.PROFILES:
            if c.holds[p] is not None:
                groups.setdefault((c.group, p), set()).add(c.holds[p])
    assert groups
    # (the fused pass under imageproc: a width of R + 2 = 9 is below the 10
    # columns of 2 kImageBorder, so only the OpenCV radius has a false side)
    for key, sides in groups.items():
        if key == ("fused", K.IMAGEPROC):
            assert sides == {True}
            continue
        assert sides == {True, False}, key


def test_seed_and_pair_cases_are_on_the_threshold():
    """One step: seed widths 158 / 160 / 162 and heights 62 / 64 / 66; pair
    widths and heights 63 / 64 / 65."""
    seed = {K.octave_sizes(c.w, c.h)[0] for c in K.CASES if c.kind == "seed"}
    assert {(158, 80), (160, 80), (162, 80), (160, 62), (160, 64), (160, 66), (158, 64)} <= seed
    pair = {K.octave_sizes(c.w, c.h)[1] for c in K.CASES if c.kind == "pair"}
    assert {(63, 400), (64, 400), (65, 400), (400, 63), (400, 64), (63, 64), (64, 63), (64, 64)} <= pair
    for c in K.CASES:
        if c.kind == "pair":  # the octave is below the tail under the case's options
            for p in K.PROFILES:
                assert c.tail[p] > 1, (c.name, p)


@pytest.mark.parametrize("profile", K.PROFILES)
def test_strip_cases_cover_r_and_r_plus_1(profile):
    """Under tail = 0 every blur radius of the profile meets an octave whose
    smaller side is R + 1 (the strip kernel, one reflection exactly) and one
    whose smaller side is R (the tile kernel)."""
    seen = set()
    for c in K.CASES:
        if c.kind != "strip":
            continue
        for o, s, R, W, H, fam in K.blur_families(c.w, c.h, profile, K.OPTION_SETS[c.opts]):
            assert fam == ("strip" if min(W, H) > R else "tile")
            seen.add((R, min(W, H) - R, fam))
            if W != H:
                seen.add((R, min(W, H) - R, "w" if W < H else "h"))
    for R in set(K.OCT_R[profile][1:]):
        assert (R, 1, "strip") in seen and (R, 0, "tile") in seen, (R, sorted(seen))
    # the last blur's radius also on a width alone and on a height alone
    R = K.OCT_R[profile][5]
    assert {(R, 1, "w"), (R, 0, "w"), (R, 1, "h"), (R, 0, "h")} <= seen, sorted(seen)


def test_seam_cases_straddle_the_strip_width():
    """Octave widths of k strips - 1, k strips, k strips + 1 column for the
    128-column strips and the 112- / 120-column pair strips, in an octave that
    takes that family under one of the case's option sets."""
    for T, profile, ws in [(K.STRIP_TW, K.OPENCV, (127, 128, 129, 257)), (K.STRIP_TW, K.IMAGEPROC, (127, 128, 129, 257)),
                           (K.PAIR_TWO[K.OPENCV], K.OPENCV, (111, 112, 113, 224, 225)),
                           (K.PAIR_TWO[K.IMAGEPROC], K.IMAGEPROC, (119, 120, 121, 240))]:
        rem = set()
        for w in ws:
            for h in (40, 64):
                c = K.BY_NAME[f"seam_{w}x{h}"]
                for name in K.pyramid_option_sets(c):
                    opts = K.OPTION_SETS[name]
                    sizes = K.octave_sizes(w, h)
                    o_tail = K.tail_octave_start(sizes, profile, opts.get("tail", 1))
                    for o in range(min(o_tail, 2)):
                        W, H = sizes[o]
                        if T == K.STRIP_TW or K.pair_applies(W, H, opts):
                            rem.add((W - 1) % T + 1 if W % T in (0, 1, T - 1) else None)
        assert {T - 1, T, 1} <= rem, (T, profile, rem)


def test_fused_cases_straddle_the_wave_width():
    for cols in (K.DR_COLS, K.BD2_COLS):
        rem = set()
        for c in K.CASES:
            if c.kind == "fused":
                for W, H in K.octave_sizes(c.w, c.h)[:2]:
                    rem.add(W % cols)
        assert {cols - 1, 0, 1} <= rem, (cols, rem)
    assert {31, 32, 33} <= {K.octave_sizes(c.w, c.h)[1][1] for c in K.CASES if c.kind == "fused"}
    # with tail = 0 the pass takes octaves 0 and 1 of every fused case
    for c in K.CASES:
        if c.kind == "fused":
            for p in K.PROFILES:
                assert K.fused_octaves(c.w, c.h, p, K.DETECT_MODES["pair_notail"])[:2] == [0, 1], (c.name, p)


def test_row_cases_straddle_the_segment_count():
    """strip_segment_rows gives rows / 40 segments at these sizes: the octave-0
    heights of the row cases sit on both sides of 80 and of 160 rows."""
    nseg = {2 * c.h: K.strip_segments(2 * c.h, (2 * c.w + K.STRIP_TW - 1) // K.STRIP_TW)[1]
            for c in K.CASES if c.kind == "rows"}
    assert nseg == {78: 1, 80: 2, 82: 2, 158: 3, 160: 4, 162: 4}


DETECT = [c for c in K.CASES if c.detect]


@pytest.mark.parametrize("profile", K.PROFILES)
@pytest.mark.parametrize("case", DETECT, ids=_ids(DETECT))
def test_enough_keypoints(oracle, case, profile):
    n = sum(len(r[0]) for r in _oracle(oracle, case, profile).values())
    assert n >= (50 if case.w * case.h >= 3000 else 1), n


SEAMS = [c for c in K.CASES if c.seam]


@pytest.mark.parametrize("case", SEAMS, ids=_ids(SEAMS))
def test_extremum_at_the_seam(oracle, case):
    o, col = case.seam
    W, H = K.octave_sizes(case.w, case.h)[o]
    assert K.K_IMAGE_BORDER < col < W - K.K_IMAGE_BORDER  # an extremum can lie there
    for p in case.seam_profiles:
        near = 0
        for kp, desc, ext in _oracle(oracle, case, p).values():
            if len(ext):
                near += int(((ext[:, 0] == o) & (np.abs(ext[:, 4] - col) <= 1)).sum())
        assert near >= 1, (p, near)
