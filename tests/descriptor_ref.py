"""The rule that compares descriptor bytes with the f64 reference, and the
fixtures it is applied to.

The reference is oracle.compute_descriptor_f64 (oracle/descriptor_body.inc,
double instance): the reference's compute_descriptor on the same f32 plane and
f32 keypoint fields with every operation in double, giving the 128 values
v = flat * norm before rounding and the 255 saturation.  A producer of u8
descriptors (the f32 oracle, describe.hip's fast or exact path) is held to v
byte by byte, except inside a band of half-width delta around the .5
boundaries, where either neighbouring byte is accepted.

A helper module (imported by test_descriptor_ref_cpu.py and
test_gpu_descriptor_f64.py), not a conftest.
"""
from collections import namedtuple

import numpy as np

import patterns

# The widest band any producer may be granted: with it the undecided share of
# the reference alone stays <= MAX_UNDECIDED on every fixture (a condition on
# the fixtures, asserted by test_descriptor_ref_cpu.py).
DELTA_CAP = 1e-2
MAX_UNDECIDED = 0.03
# The f32 oracle's own band (test_descriptor_ref_cpu.py: measured <= 1.2e-5).
DELTA_F32 = 1e-4

Check = namedtuple("Check", "violations undecided_share implied_deviation")


def check(bytes_u8, v_f64, delta):
    """Hold u8 descriptor bytes to the unrounded f64 values `v_f64`.

    r = min(floor(v + 0.5), 255); dist = |v - floor(v) - 0.5|.  A byte is
    decided when dist > delta or v >= 255.5; a decided byte must equal r, an
    undecided one must be floor(v) or floor(v) + 1 (both clamped to 255).

    Returns Check(violations, undecided_share, implied_deviation): the flat
    indices of the bytes that break the rule, the share of undecided bytes,
    and the largest dist among the bytes that differ from r -- a lower bound,
    in byte steps, on the producer's error (0.0 when none differs; for a byte
    under a saturated v >= 255.5 the distance v - 254.5 to the nearest value
    that rounds below 255)."""
    b = np.asarray(bytes_u8).astype(np.int64).ravel()
    v = np.asarray(v_f64, np.float64).ravel()
    assert b.shape == v.shape, (b.shape, v.shape)
    if b.size == 0:
        return Check(np.zeros(0, np.int64), 0.0, 0.0)
    assert np.all(np.isfinite(v)) and v.min() >= 0.0
    f = np.floor(v)
    r = np.minimum(np.floor(v + 0.5), 255.0).astype(np.int64)
    dist = np.abs(v - f - 0.5)
    saturated = v >= 255.5
    decided = (dist > delta) | saturated
    lo = np.minimum(f, 255.0).astype(np.int64)
    hi = np.minimum(f + 1.0, 255.0).astype(np.int64)
    ok = np.where(decided, b == r, (b == lo) | (b == hi))
    differs = b != r
    dev = np.where(saturated, v - 254.5, dist)
    implied = float(dev[differs].max()) if differs.any() else 0.0
    return Check(np.flatnonzero(~ok), float((~decided).mean()), implied)


def byte_contract(bytes_u8, ref_u8):
    """test_gpu_parity.assert_parity's descriptor clause, as a predicate:
    max |d| <= 1 per byte and >= 99 % of the bytes identical."""
    dd = np.abs(np.asarray(bytes_u8).astype(np.int32) - np.asarray(ref_u8).astype(np.int32))
    return bool(dd.size == 0 or (dd.max() <= 1 and (dd == 0).mean() >= 0.99))


# ---- fixtures --------------------------------------------------------------

PARITY = ["bird_small", "tree_small", "synth_301x207", "synth_97x61"]  # test_gpu_parity's, less the two large ones
WALK = ["ramp_dir0", "ramp_dir03", "ramp_dir45", "clip_dir0", "clip_dir03", "clip_dir45"]
# CPU only (test_descriptor_ref_cpu.py): the second image of the variant counts
CPU_ONLY = ["synth_640x480"]


def pattern_names(profile):
    """The tests/patterns.py patterns that yield keypoints in `profile`."""
    from test_patterns_cpu import COUNTS
    return [n for n in patterns.names() if COUNTS[n][profile] > 0]


def fixtures(profile):
    return PARITY + WALK + pattern_names(profile)


_images = {}


def image(name):
    """The named fixture as a read-only u8 array (built once)."""
    if name not in _images:
        if name in patterns.REGISTRY:
            a = patterns.make(name)
        elif name in WALK:
            import test_gpu_describe_walk
            a = test_gpu_describe_walk.make(name)
        elif name.startswith("synth_"):
            import synth
            w, h = map(int, name.split("_")[1].split("x"))
            a = synth.frame(w, h, {"synth_640x480": 3, "synth_301x207": 11, "synth_97x61": 5}[name])
        else:
            from conftest import load_golden
            a = load_golden(name)["image"]
        a = np.ascontiguousarray(a, dtype=np.uint8)
        a.setflags(write=False)
        _images[name] = a
    return _images[name]


_pyramids = {}
_refs = {}


def reference(oracle, name, profile, variant=0):
    """The oracle's (keypoints, descriptors, internal keys, f64 descriptors) of
    a fixture: computed once per (name, profile, variant), shared, read-only.
    A descriptor variant (oracle.VARIANT_DESC_*) changes the u8 descriptors
    only: it reuses variant 0's pyramid, keypoints and f64 values."""
    key = (name, profile, variant)
    if key not in _refs:
        if variant == 0:
            r = oracle.sift(image(name), profile=profile, internal=True, desc_f64=True)
        else:
            kp, _, ext, v = reference(oracle, name, profile)
            if (name, profile) not in _pyramids:
                _pyramids[name, profile] = oracle.Pyramid(image(name), profile)
            with oracle.set_variant(variant):
                kp_v, desc_v = _pyramids[name, profile].sift_with_precomputed()
            assert np.array_equal(kp_v.view(np.uint32), kp.view(np.uint32))  # descriptor variants move no keypoint
            r = (kp, desc_v, ext, v)
        for a in r:
            a.setflags(write=False)
        _refs[key] = r
    return _refs[key]
