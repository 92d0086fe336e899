"""The fast descriptor path's band walk and one-pass histogram scatter
(describe.hip, describe_wave_fast) on images built to provoke what it must
not do: lose an update when two lanes of one histogram slice hit the same
slots in one LDS instruction.

Single-orientation windows: a triangle-wave ramp gives every descriptor
window a nearly constant gradient direction, so two samples in the same 2x2
cell footprint are also in the same orientation bin pair -- every same-cell
pair of slice partners is a hazard the kernel has to detect and send through
the four-round form.  Seeded Gaussian blobs on top of the ramp give keypoints
over octaves 0-5 with sizes ~1.1-35 (64-77 per image), i.e. window rows from
a few to ~80 samples.  Clipped windows: the same on 80x80 with the blobs next to the
borders, where the sample list is cut short and the bands of a window are no
longer a quarter of a window apart.

A lost update is ~7e-4 of a bin: a few of them move a descriptor byte, and
systematic ones cost whole percent of the identical-byte share.  The bounds
are test_gpu_parity.assert_parity's (|d| <= 1 per byte, >= 99 % of the bytes
identical to the oracle) and, against the bit-exact mode, the share measured
before the walk changed.
"""
import numpy as np
import pytest

from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

DIRECTIONS = {"dir0": (0.0, 0.8), "dir03": (0.3, 1.0), "dir45": (np.pi / 4, 1.3)}  # ramp direction (rad), slope


def ramp_blobs(size, direction, slope, seed, border=None):
    """u8 image: triangle-wave ramp (period 200 px, `slope` grey levels per px
    along `direction`) + 60 Gaussian blobs (sigma 1.2-7 px, amplitude +-40-90)
    + 60, clipped.  border: blob centres within that many px of an image edge."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    t = xx * np.cos(direction) + yy * np.sin(direction)
    img = slope * (100.0 - np.abs(np.mod(t, 200.0) - 100.0)) + 60.0
    for _ in range(60):
        if border is None:
            cx, cy = rng.uniform(0, size, 2)
        else:
            along, d = rng.uniform(0, size), rng.uniform(0, border)
            side = rng.randint(4)
            cx, cy = [(along, d), (along, size - 1 - d), (d, along), (size - 1 - d, along)][side]
        sigma = rng.uniform(1.2, 7.0)
        amp = rng.uniform(40.0, 90.0) * (1.0 if rng.randint(2) else -1.0)
        img += amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * sigma * sigma))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def make(name):
    kind, d = name.split("_")
    direction, slope = DIRECTIONS[d]
    seed = 1000 + sorted(DIRECTIONS).index(d)
    return ramp_blobs(256, direction, slope, seed) if kind == "ramp" else ramp_blobs(80, direction, slope, seed, 12)


RAMPS = ["ramp_" + d for d in DIRECTIONS]
CLIPPED = ["clip_" + d for d in DIRECTIONS]

# Share of descriptor bytes on which the default path equals the exact mode,
# measured with the row-major walk and four-round scatter this file's kernel
# replaced (same images, MI355X); every other byte differed by 1.
PARENT_SHARE = {  # 64 / 74 / 77 and 18 / 16 / 15 keypoints: not one byte differed
    "ramp_dir0": 1.0, "ramp_dir03": 1.0, "ramp_dir45": 1.0,
    "clip_dir0": 1.0, "clip_dir03": 1.0, "clip_dir45": 1.0,
}

_memo = {}


def _oracle(oracle, name):
    """The oracle's result for an image: computed once, shared, read-only."""
    if name not in _memo:
        r = oracle.sift(make(name), internal=True)
        for a in r:
            a.setflags(write=False)
        _memo[name] = r
    return _memo[name]


@pytest.fixture(scope="module")
def exact_ctx(pkg):
    c = pkg.Context(0, pkg.OpenCVProcessing)
    c.set_exact_descriptors(True)
    yield c
    c.close()


def _report(tag, name, got, want):
    dd = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"\nWALK {tag} {name}: n {len(got)} identical-byte share {(dd == 0).mean():.5f} max|d| {dd.max()}")
    return dd


@pytest.mark.parametrize("name", RAMPS)
def test_single_orientation_windows(pkg, ctx, oracle, name):
    kp_o, desc_o, ext_o = _oracle(oracle, name)
    assert len(kp_o) >= 50, len(kp_o)  # a precondition on the oracle's result
    res = ctx.sift(make(name))
    if len(res) == len(kp_o):
        _report("oracle", name, res.descriptors, desc_o)
    assert_parity(pkg, res, kp_o, desc_o, ext_o)


@pytest.mark.parametrize("name", CLIPPED)
def test_clipped_windows(pkg, ctx, oracle, name):
    kp_o, desc_o, ext_o = _oracle(oracle, name)
    assert len(kp_o) > 0
    res = ctx.sift(make(name))
    if len(res) == len(kp_o):
        _report("oracle", name, res.descriptors, desc_o)
    assert_parity(pkg, res, kp_o, desc_o, ext_o)


@pytest.mark.parametrize("name", ["ramp_dir03", "clip_dir45"])
def test_deterministic(ctx, name):
    """Two runs byte-identical; a frame alone and inside a 3-frame batch too."""
    img = make(name)
    a, b = ctx.sift(img), ctx.sift(img)
    assert len(a) > 0
    assert a == b and np.array_equal(a.descriptors, b.descriptors)
    other = make("ramp_dir0" if name.startswith("ramp") else "clip_dir0")
    batch = ctx.sift_batch(np.stack([other, img, other]))
    assert len(batch[1]) == len(a)
    assert np.array_equal(batch[1].keypoints_array, a.keypoints_array)
    assert np.array_equal(batch[1].descriptors, a.descriptors)
    assert np.array_equal(batch[0].descriptors, batch[2].descriptors)


@pytest.mark.parametrize("name", RAMPS + CLIPPED)
def test_default_against_exact(ctx, exact_ctx, name):
    """|d| <= 1 per byte, and the identical share not below the parent's on
    the same image minus 0.1 percentage point."""
    img = make(name)
    fast, exact = ctx.sift(img), exact_ctx.sift(img)
    assert len(fast) == len(exact) > 0
    assert np.array_equal(fast.keypoints_array, exact.keypoints_array)
    dd = _report("exact", name, fast.descriptors, exact.descriptors)
    assert dd.max() <= 1, dd.max()
    assert (dd == 0).mean() >= PARENT_SHARE[name] - 0.001, ((dd == 0).mean(), PARENT_SHARE[name])
