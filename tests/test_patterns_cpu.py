"""The structured patterns (tests/patterns.py) on the CPU oracle alone.

Three things are pinned here, so that the argument for the GPU tests of
test_gpu_patterns.py can be repeated without a GPU:

  * each of the oracle's three deliberately wrong variants (sift_oracle.c
    oracle_set_variant bits 256 / 512 / 1024: strict extremum comparisons,
    half-up orientation bin, f32 atan2f orientation angle) changes the result
    on at least one registered pattern, in both profiles -- so a kernel with
    the same mistake fails test_pattern_parity;
  * none of them changes anything on the inputs the suite had before
    (synth, noise, bird_small) -- the gap these patterns close;
  * every pattern keeps the property it is there for (exact keypoint counts,
    tied responses, many orientations, plateaus, |dx| = |dy| gradients).

Variant 0 is what tests/test_oracle_golden.py pins.
"""
import numpy as np
import pytest
from conftest import load_golden

import patterns

WRONG = {"strict_extremum": 256, "half_up_bin": 512, "f32_atan2": 1024}

_memo = {}


def _oracle(oracle, img_key, img, profile, variant=0):
    key = (img_key, profile, variant)
    if key not in _memo:
        with oracle.set_variant(variant):
            _memo[key] = oracle.sift(img, profile=profile, internal=True)
    return _memo[key]


def _differs(a, b):
    """A changed count, or any changed keypoint or descriptor byte."""
    return (len(a[0]) != len(b[0]) or not np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
            or not np.array_equal(a[1], b[1]))


def test_set_variant_resets(oracle):
    img = patterns.make("checker5")
    base = _oracle(oracle, "checker5", img, 0)
    with pytest.raises(RuntimeError):
        with oracle.set_variant(256):
            raise RuntimeError("leave the block by an exception")
    assert not _differs(oracle.sift(img, internal=True), base)  # back to variant 0


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("variant", list(WRONG))
def test_wrong_variant_is_caught(oracle, variant, profile):
    """For each wrong variant and profile at least one registered pattern
    gives a result that differs from variant 0."""
    caught = [n for n in patterns.names()
              if _differs(_oracle(oracle, n, patterns.make(n), profile),
                          _oracle(oracle, n, patterns.make(n), profile, WRONG[variant]))]
    print(f"{variant} profile {profile}: caught by {caught}")
    assert caught, f"no registered pattern distinguishes the {variant} variant in profile {profile}"


@pytest.mark.parametrize("profile", [0, 1])
def test_strict_extremum_changes_counts(oracle, profile):
    """The tie patterns of the extremum test, by keypoint count.  OpenCV
    profile: checker5 3188 -> 220.  Imageproc profile: a search over checker
    periods 4-9 and block sizes 3-9 (both frame shapes) found no count change
    above 4 (blocks of 5: 454 -> 450); even-sided squares do better, and
    `squares12` (period 12, side 8) is registered for it: 755 -> 715
    (OpenCV profile 980 -> 524).  `bigsq` stays as the minimal case, 4 -> 2."""
    def count(name, variant):
        return len(_oracle(oracle, name, patterns.make(name), profile, variant)[0])
    if profile == 0:
        assert (count("checker5", 0), count("checker5", 256)) == (3188, 220)
        assert (count("squares12", 0), count("squares12", 256)) == (980, 524)
    else:
        assert (count("squares12", 0), count("squares12", 256)) == (755, 715)
        assert (count("bigsq", 0), count("bigsq", 256)) == (4, 2)
    assert count("squares12", 0) - count("squares12", 256) >= 10


def _old_inputs():
    import synth
    return {"synth_301x207": synth.frame(301, 207, 11),
            "noise_96x128": np.random.default_rng(5).integers(0, 256, (96, 128), dtype=np.uint8),
            "bird_small": load_golden("bird_small")["image"]}


@pytest.mark.parametrize("profile", [0, 1])
def test_old_inputs_do_not_catch_the_variants(oracle, profile):
    """Documentation of the gap: on the inputs the suite had before the
    patterns, the three wrong variants are bit-identical to variant 0."""
    for name, img in _old_inputs().items():
        base = _oracle(oracle, name, img, profile)
        assert len(base[0]) > 0
        for vname, bits in WRONG.items():
            assert not _differs(base, _oracle(oracle, name, img, profile, bits)), (
                f"{name} (profile {profile}) now distinguishes the {vname} variant: the gap the structured "
                "patterns were added for has closed some other way; this assertion documents it and can go")


# exact oracle keypoint counts (OpenCV, imageproc); the oracle is deterministic
COUNTS = {
    "checker5": (3188, 168), "checker8": (562, 1882), "squares": (572, 547), "squares12": (980, 755),
    "diamonds": (463, 497), "tiled32": (1282, 1162), "sym4": (301, 257), "satblobs": (71, 56),
    "rings": (15, 13), "blocks4": (394, 348), "blocks6": (309, 738), "bigsq": (2, 4), "edge_dots": (4, 8),
    "white": (0, 0), "step": (0, 0), "stars_inv": (0, 0), "diag7": (1, 0),
    "white_96x128": (0, 0), "step_96x128": (0, 0), "flat77_96x128": (0, 0),
    "border_mosaic": (455, 429), "drift_mosaic": (338, 346), "streaks13": (100, 85),
}


def test_every_pattern_has_a_count():
    assert set(COUNTS) == set(patterns.names())
    assert set(patterns.ZERO_KEYPOINTS) == {n for n, c in COUNTS.items() if c == (0, 0)}


@pytest.mark.parametrize("name", list(COUNTS))
def test_pattern_counts(oracle, name):
    img = patterns.make(name)
    assert img.dtype == np.uint8 and img.shape == patterns.REGISTRY[name][:2]
    got = tuple(len(_oracle(oracle, name, img, p)[0]) for p in (0, 1))
    assert got == COUNTS[name]


def test_edge_dots_keypoints_hug_the_border(oracle):
    img = patterns.make("edge_dots")
    h, w = img.shape
    kp = _oracle(oracle, "edge_dots", img, 1)[0]
    d = np.minimum(np.minimum(kp[:, 0], w - 1 - kp[:, 0]), np.minimum(kp[:, 1], h - 1 - kp[:, 1]))
    assert len(kp) == 8 and d.max() <= 6.0, d


def test_tied_responses(oracle):
    """features_limit has ties to cut: checker5 (OpenCV) holds one group of
    >= 1000 bit-equal responses, tiled32 >= 40 groups (both profiles)."""
    kp = _oracle(oracle, "checker5", patterns.make("checker5"), 0)[0]
    groups, _ = patterns.response_groups(kp[:, 4])
    assert max(b - a for a, b in groups) >= 1000
    for profile in (0, 1):
        kp = _oracle(oracle, "tiled32", patterns.make("tiled32"), profile)[0]
        assert len(patterns.response_groups(kp[:, 4])[0]) >= 40
    for name in ("squares", "diamonds"):  # the other two test_pattern_limit_cuts_a_tie uses
        kp = _oracle(oracle, name, patterns.make(name), 0)[0]
        assert max(b - a for a, b in patterns.response_groups(kp[:, 4])[0]) >= 2


def test_rings_many_orientations(oracle):
    """One extremum with >= 7 orientation peaks (synth rarely exceeds 2)."""
    for profile in (0, 1):
        ext = _oracle(oracle, "rings", patterns.make("rings"), profile)[2]
        _, per = np.unique(ext[:, [0, 2, 3, 4]], axis=0, return_counts=True)
        assert per.max() >= 7, per.max()


def _tied_extrema(dog):
    """Pixels of one octave's DoG stack (5, h, w) that pass
    point_is_local_extremum (src/lib.rs:437-506: non-strict, threshold 0,
    border 5) with at least one of the 26 neighbours equal to them."""
    n = 0
    B = 5
    h, w = dog.shape[1:]
    if h < 2 * B or w < 2 * B:
        return 0
    for s in (1, 2, 3):
        val = dog[s, B:h - B, B:w - B]
        mx = np.full(val.shape, -np.inf, np.float32)
        mn = np.full(val.shape, np.inf, np.float32)
        eq = np.zeros(val.shape, bool)
        for ds in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if ds == dy == dx == 0:
                        continue
                    nb = dog[s + ds, B + dy:h - B + dy, B + dx:w - B + dx]
                    mx = np.maximum(mx, nb)
                    mn = np.minimum(mn, nb)
                    eq |= nb == val
        ext = ((val > 0) & (val >= mx)) | ((val < 0) & (val <= mn))
        n += int((ext & eq).sum())
    return n


@pytest.mark.parametrize("name", ["white", "step", "stars_inv"])
def test_plateau_candidates(oracle, name):
    """Zero keypoints, but the blurs' rounding plateaus pass the extremum test
    on a tie: the candidate buffer's worst case.  More than 50 000 octave
    pixels do so in the imageproc profile (white 163 527, step 69 779,
    stars_inv 65 266) and on `white` in the OpenCV profile (73 645); `step`
    and `stars_inv` have 31 328 and 23 825 there (the half of `step` that is
    exactly 0 fails |val| > 0).  Every count is far above a fresh context's
    candidate bound for a 97 x 161 frame, 1.3 * sum(px) / 256 + 1024 = 1446
    (pipeline.cpp chunk_bounds), which is what test_pattern_first_call_bounds
    relies on."""
    counts = []
    for profile in (0, 1):
        pyr = oracle.Pyramid(patterns.make(name), profile)
        counts.append(sum(_tied_extrema(pyr.dog(o)) for o in range(pyr.n_octaves)))
    print(f"{name}: {counts} tied extremum pixels (OpenCV, imageproc)")
    assert counts[1] > 50000, counts
    if name == "white":
        assert counts[0] > 50000, counts
    h, w = patterns.make(name).shape
    first_call_bound = 1.3 * (4 * h * w * 4 / 3) / 256 + 1024  # sum over octaves of px <= 4/3 of octave 0's
    assert min(counts) > 10 * first_call_bound, (counts, first_call_bound)


@pytest.mark.parametrize("name", ["squares", "diamonds"])
def test_gradient_ties(oracle, name):
    """>= 1 % of the non-zero gradient samples of G_1..G_3 have |dx| = |dy|:
    the orientation angle lands on a bin boundary's neighbourhood (the
    kernel's deferral to a correctly rounded f64 atan2, detect.hip k_orient)."""
    pyr = oracle.Pyramid(patterns.make(name), 0)
    tied = nonzero = 0
    for o in range(pyr.n_octaves):
        g = pyr.scale_space(o)[1:4]
        if g.shape[1] < 3 or g.shape[2] < 3:
            continue
        dx = g[:, 1:-1, 2:] - g[:, 1:-1, :-2]
        dy = g[:, :-2, 1:-1] - g[:, 2:, 1:-1]
        nz = (dx != 0) | (dy != 0)
        nonzero += int(nz.sum())
        tied += int((nz & (np.abs(dx) == np.abs(dy))).sum())
    print(f"{name}: {tied} of {nonzero} non-zero gradient samples tied ({tied / nonzero:.4f})")
    assert tied >= 0.01 * nonzero, (tied, nonzero)
