"""The pair strips' two-slot G_s ring (blur2_body, pyramid.hip) against the
CPU oracle.

k_seed_pair and k_blur2_strip keep the intermediate plane G_s of a blur pair
in a ring of two LDS slots: chunk k shares its slot with chunk k - 2, and
column pass A's rows of chunk k wait in registers until column pass B has
read chunk k - 2.  A slot overwritten one phase early, a deferred write that
is dropped or lands in the other slot, or one mishandled at the first / last
steps of a segment, puts stale or shifted rows into G_{s+1} of some chunks of
some segments.  The shapes below give segments of 3, 4, 5 and 7 sixteen-row
chunks (both ring parities, one to three wraps, last chunks partly outside
the segment), more than one strip (the left / right fixup columns) and more
than one segment per plane; the images are seeded u8 noise
(kernel_shapes.noise), where a stale or shifted row cannot cancel.

Compared bit for bit: G_0 .. G_3 of octave 0 (k_seed_pair writes G_0, G_1;
the (2, 3) pair G_2, G_3 and octave 1's base) and G_1, G_2 of octave 1 (the
(1, 2) pair), for both profiles.  No tolerance.

The last test runs the two-column fused blur-5 + scan pass (k_blur_detect_pair)
forced onto every octave of a 248x48 frame and compares its keypoints with
the separate blur + scan kernels'.
"""
import numpy as np
import pytest

import kernel_shapes as K

pytestmark = pytest.mark.gpu

CHUNK = 16  # rows per chunk of the pair strips (PairGeom: StripGeom<R, 16>)

# (frame w, frame h, frames in the chunk) -> (segments, output chunks per
# segment) of octave 0 under the segment rule (kernel_shapes.strip_segments),
# the same for both profiles' strip counts
SHAPES = {
    (80, 32, 1): (1, 4),     # 160 x 64: one segment of 64 rows
    (113, 40, 1): (2, 3),    # 226 x 80: two segments of 40 rows, the last chunk half outside
    (80, 33, 1): (1, 5),     # 160 x 66: one segment of 66 rows, 2 rows in the last chunk
    (120, 130, 1): (6, 3),   # 240 x 260: six segments of 44 rows; octave 1 (120 x 130) three of 44
    (113, 40, 3): (2, 3),    # three frames in one chunk: tile.z > 0
    # 368 x 200, 4 strips x 256 frames = 1024 workgroups per segment row: the
    # rule stops at two segments of 100 rows (seven chunks, 4 rows in the last)
    (184, 100, 256): (2, 7),
}


def _processing(pkg, profile):
    return pkg.OpenCVProcessing if profile == K.OPENCV else pkg.ImageprocProcessing


def _segments(w0, h0, n, profile):
    strips = (w0 + K.PAIR_TWO[profile] - 1) // K.PAIR_TWO[profile]
    seg, nseg = K.strip_segments(h0, strips * n, 8192)
    return strips, nseg, (seg + CHUNK - 1) // CHUNK


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} values differ, rows {bad[:, 0].min()}..{bad[:, 0].max()}, "
                             f"columns {bad[:, 1].min()}..{bad[:, 1].max()}, first (y, x) {bad[:5].tolist()}")


def _check(planes, opy, what):
    """planes[o]: (6, h, w) of octave o."""
    assert opy.n_octaves >= 2
    for o, blurs in ((0, (0, 1, 2, 3)), (1, (1, 2))):
        want = opy.scale_space(o)
        for s in blurs:
            _same(planes[o][s], want[s], f"{what} octave {o} G_{s}")


@pytest.mark.parametrize("profile", K.PROFILES)
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "%dx%dx%d" % s)
def test_pair_ring_planes(pkg, oracle, shape, profile):
    w, h, n = shape
    (w0, h0), (w1, h1) = K.octave_sizes(w, h)[:2]
    assert K.seed_pair_applies(w0, h0) and K.pair_applies(w0, h0)
    strips, nseg, chunks = _segments(w0, h0, n, profile)
    assert strips > 1 and (nseg, chunks) == SHAPES[shape]
    c = pkg.Context(0, _processing(pkg, profile))
    # tail = 0: the small shapes' octaves would otherwise all go to
    # k_octave_tail (imageproc 80x32) and no pair kernel would run
    c.set_path_option("tail", 0)
    try:
        if n == 1:
            img = K.noise(w, h)
            c.reset_stats()
            pre = c.precompute_images(img)
            assert c.stats()["pyramid_launches"] == K.dispatch(w, h, profile, {"tail": 0})[1]
            _check([pre.scale_space_octave(o) for o in (0, 1)], oracle.Pyramid(img, profile), f"{w}x{h}")
            return
        base = K.noise(w, h * n).reshape(n, h, w)
        c.set_chunk(n)
        c.sift_batch(base)
        for i in sorted({0, n // 2, n - 1}):
            planes = [c.read_batch_scale_space(i, 0, (w0, h0)), c.read_batch_scale_space(i, 1, (w1, h1))]
            _check(planes, oracle.Pyramid(base[i], profile), f"{w}x{h} frame {i} of {n}")
    finally:
        c.close()


def test_fused_pair_scan_same_keypoints(pkg):
    """fused_detect = 2, bd_pair = 1, tail = 0 on a 248x48 frame (octave 0:
    four 124-column waves; octave 1: two; 32-row segments): the same
    keypoints as the separate blur 5 and k_detect_rows."""
    img = K.noise(248, 48)
    c = pkg.Context(0, pkg.OpenCVProcessing)
    try:
        with c.path_options(fused_detect=2, bd_pair=1, tail=0):
            c.reset_stats()
            fused = c.sift(img)
            st = c.stats()
        with c.path_options(fused_detect=0, tail=0):
            apart = c.sift(img)
    finally:
        c.close()
    sizes = K.octave_sizes(248, 48)
    ran = K.fused_octaves(248, 48, K.OPENCV, {"fused_detect": 2, "tail": 0})
    assert ran and st["pyramid_scan_bytes"] == 20 * sum(sizes[o][0] * sizes[o][1] for o in ran)
    assert len(fused) == len(apart) and len(fused) > 0
    assert np.array_equal(fused.keys, apart.keys)
    assert np.array_equal(fused.keypoints_array, apart.keypoints_array)
    assert np.array_equal(fused.descriptors, apart.descriptors)
