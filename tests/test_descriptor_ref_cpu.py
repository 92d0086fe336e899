"""The f64 descriptor reference and the byte rule of tests/descriptor_ref.py,
on the CPU oracle alone.

What is pinned here, so that test_gpu_descriptor_f64.py's argument can be
repeated without a GPU:

  * the float instance of oracle/descriptor_body.inc is still the oracle's
    compute_descriptor: the golden snapshots agree as test_oracle_golden.py
    demands, and the descriptor bytes of the parity and walk fixtures have the
    digests recorded before the body was written over a real type;
  * the f32 oracle passes the rule at delta = 1e-4 on every fixture, in both
    profiles (measured: implied deviation <= 1.2e-5 OpenCV profile, <= 2.9e-5
    imageproc) -- f32 rounding is four orders of magnitude below a byte step;
  * the reference alone leaves <= 3 % of the bytes undecided at DELTA_CAP on
    every fixture (a condition on the fixtures);
  * each of the five wrong-on-purpose descriptor variants (oracle_set_variant
    bits 2048..32768), used as the producer, is rejected by the rule at
    DELTA_CAP and at the GPU test's DELTA_FAST -- while assert_parity's byte
    contract alone passes them (printed; README, "Correctness").
"""
import hashlib

import numpy as np
import pytest
from conftest import load_golden

import descriptor_ref as D
from test_gpu_descriptor_f64 import DELTA_FAST

SMALL = {"exp_const": 2048, "mag_half": 4096, "ori_bias": 8192}  # a few 1e-2 of a byte step
STRUCTURAL = {"lost_sample": 16384, "no_wrap": 32768}  # one contribution, or one bin pair, missing

# sha256 of the f32 oracle's (n, 128) u8 descriptors, recorded with
# oracle_compute_descriptor as it was before descriptor_body.inc (first 16 hex
# digits; OpenCV, imageproc profile)
DIGESTS = {
    "bird_small": ("4b5d212dbfaf94a5", "a90ba2900920ed5d"),
    "tree_small": ("1e21d8de7e7c8bb2", "aabd91a7a2d0a0f7"),
    "synth_301x207": ("956250100ac18634", "1eb5c8c171d072e9"),
    "synth_97x61": ("17f517d1aae62bed", "117ecf9d022e53bd"),
    "ramp_dir0": ("b0165c39a2bc824d", "34cde32fad5c59f8"),
    "ramp_dir03": ("4c4d6827f6d05884", "0f98bd712d6b43ae"),
    "ramp_dir45": ("14a2d29673aeb25a", "40964eef03837d83"),
    "clip_dir0": ("a4e7979297baf95c", "b3baf5ef290ebabd"),
    "clip_dir03": ("350d2ccd82db0480", "ad069a645fb5f2fe"),
    "clip_dir45": ("ac2ab378eaf645e3", "1383a9fd4be66acd"),
    "synth_640x480": ("c7d4f367b1ca9f44", "48924ceda142261f"),
}


def _digest(desc):
    return hashlib.sha256(np.ascontiguousarray(desc).tobytes()).hexdigest()[:16]


def test_variant_constants(oracle):
    assert (oracle.VARIANT_DESC_EXP_CONST, oracle.VARIANT_DESC_MAG_HALF, oracle.VARIANT_DESC_ORI_BIAS,
            oracle.VARIANT_DESC_LOST_SAMPLE, oracle.VARIANT_DESC_NO_WRAP) == (2048, 4096, 8192, 16384, 32768)
    assert 1e-4 <= DELTA_FAST <= D.DELTA_CAP


def test_check_rule():
    """The rule on hand-made values: decided and undecided bytes, the 255
    saturation, the implied deviation."""
    v = np.array([10.2, 10.496, 10.496, 10.496, 10.504, 254.7, 255.499, 255.6, 300.0, 0.0])
    good = np.array([10, 10, 11, 10, 11, 255, 255, 255, 255, 0], np.uint8)
    c = D.check(good, v, 1e-2)
    assert len(c.violations) == 0
    assert c.undecided_share == pytest.approx(0.5)  # the four near 10.5, and 255.499
    assert c.implied_deviation == pytest.approx(0.004)  # byte 11 under 10.496
    assert list(D.check(good, v, 1e-3).violations) == [2]  # 10.496 is decided at 1e-3
    bad = good.copy()
    bad[0], bad[3], bad[7], bad[9] = 11, 12, 254, 1
    c = D.check(bad, v, 1e-2)
    assert list(c.violations) == [0, 3, 7, 9]
    assert c.implied_deviation == pytest.approx(255.6 - 254.5)
    assert D.check(bad[[0]], v[[0]], 1e-2).implied_deviation == pytest.approx(0.3)
    empty = D.check(np.zeros((0, 128), np.uint8), np.zeros((0, 128)), 1e-2)
    assert len(empty.violations) == 0 and empty.undecided_share == 0.0 and empty.implied_deviation == 0.0
    assert D.byte_contract(good, good) and not D.byte_contract(bad, good)


@pytest.mark.parametrize("name", ["tree_small", "bird_small"])
def test_float_instance_matches_golden(oracle, name):
    from test_oracle_golden import MIN_DESC_EQUAL, golden_agreement
    g = load_golden(name)
    kp, desc, _, _ = D.reference(oracle, name, 0)
    order = oracle.stable_sort_xy_size(kp)
    _, _, desc_equal, desc_maxd = golden_agreement(kp[order], desc[order], g)
    assert desc_equal >= MIN_DESC_EQUAL and desc_maxd <= 1, (desc_equal, desc_maxd)


@pytest.mark.parametrize("name", D.PARITY + D.WALK + D.CPU_ONLY)
def test_float_instance_unchanged(oracle, name):
    got = tuple(_digest(D.reference(oracle, name, p)[1]) for p in (0, 1))
    print(f'    "{name}": {got},')
    assert got == DIGESTS[name]


def test_single_descriptor_entry_points(oracle):
    """compute_descriptor / compute_descriptor_f64 on one keypoint: the bytes
    are the rounded f32 values, and obey the rule against the f64 ones."""
    img = np.random.default_rng(3).random((96, 96), dtype=np.float32)
    for x, y, s, o in [(48.0, 48.0, 2.0, 30.0), (5.2, 90.7, 3.1, 359.9), (47.5, 48.5, 0.9, 0.0)]:
        b = oracle.compute_descriptor(img, x, y, s, o)
        v = oracle.compute_descriptor_f64(img, x, y, s, o)
        assert v.shape == (128,) and v.dtype == np.float64
        assert abs(np.sqrt((np.minimum(v, 512.0) ** 2).sum()) - 512.0) < 1e-6 * 512  # L2 = 512 before rounding
        assert len(D.check(b, v, D.DELTA_F32).violations) == 0


@pytest.mark.parametrize("profile", [0, 1])
def test_f32_oracle_under_the_rule(oracle, profile):
    worst = 0.0
    for name in D.fixtures(profile) + D.CPU_ONLY:
        kp, desc, _, v = D.reference(oracle, name, profile)
        assert len(kp) > 0 and v.shape == desc.shape, name
        c = D.check(desc, v, D.DELTA_F32)
        n_diff = int((desc != np.minimum(np.floor(v + 0.5), 255)).sum())
        print(f"F32 {name} profile {profile}: n {len(kp)} bytes off round(v) {n_diff} implied deviation "
              f"{c.implied_deviation:.2e} violations {len(c.violations)}")
        worst = max(worst, c.implied_deviation)
        assert len(c.violations) == 0, (name, c.violations[:5], c.implied_deviation)
    print(f"F32 profile {profile}: largest implied deviation {worst:.2e}")


@pytest.mark.parametrize("profile", [0, 1])
def test_undecided_share_is_capped(oracle, profile):
    """A condition on the fixtures, not a measurement: one that breaks it is
    replaced, not excused."""
    for name in D.fixtures(profile) + D.CPU_ONLY:
        _, desc, _, v = D.reference(oracle, name, profile)
        share = D.check(desc, v, D.DELTA_CAP).undecided_share
        print(f"UNDECIDED {name} profile {profile}: {share:.4f} of {desc.size} bytes")
        assert share <= D.MAX_UNDECIDED, (name, share)


def _row(oracle, name, bits):
    kp, desc, _, v = D.reference(oracle, name, 0)
    desc_v = D.reference(oracle, name, 0, bits)[1]
    old = D.byte_contract(desc_v, desc)
    c = D.check(desc_v, v, D.DELTA_CAP)
    cf = D.check(desc_v, v, DELTA_FAST)
    return old, len(c.violations), len(cf.violations), c.implied_deviation


@pytest.mark.parametrize("variant", list(SMALL))
def test_small_variant_is_rejected(oracle, variant):
    """>= 10 violating bytes on tree_small and on synth_640x480, at DELTA_CAP
    (so at any DELTA_FAST below it too)."""
    for name in ("tree_small", "synth_640x480", "synth_301x207", "bird_small"):
        old, n_cap, n_fast, dev = _row(oracle, name, SMALL[variant])
        print(f"VARIANT {variant} {name}: byte contract {'pass' if old else 'fail'}; rule violations "
              f"{n_cap} at {D.DELTA_CAP:g}, {n_fast} at {DELTA_FAST:g}; implied deviation {dev:.3f}")
        if name in ("tree_small", "synth_640x480"):
            assert n_cap >= 10 and n_fast >= n_cap, (name, n_cap, n_fast)


@pytest.mark.parametrize("variant", list(STRUCTURAL))
def test_structural_variant_is_rejected(oracle, variant):
    """>= 1 violating byte on each of at least half the fixtures."""
    names = D.fixtures(0)
    caught, passed_old = [], []
    for name in names:
        old, n_cap, n_fast, dev = _row(oracle, name, STRUCTURAL[variant])
        print(f"VARIANT {variant} {name}: byte contract {'pass' if old else 'fail'}; rule violations "
              f"{n_cap} at {D.DELTA_CAP:g}, {n_fast} at {DELTA_FAST:g}; implied deviation {dev:.3f}")
        assert n_fast >= n_cap
        if n_cap >= 1:
            caught.append(name)
        if old:
            passed_old.append(name)
    print(f"VARIANT {variant}: rule rejects it on {len(caught)} of {len(names)} fixtures; the byte contract "
          f"passes it on {len(passed_old)}")
    assert 2 * len(caught) >= len(names), (caught, names)
