"""Processing-trait ops (src/lib.rs:86-90) and compute_descriptor (src/lib.rs:785)
on the GPU vs the CPU oracle.  Blur / resize are bit-exact; compute_descriptor
within +-1 per component (LDS-atomic histogram order)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sigma", [0.6, 1.2489996, 1.2262735, 1.5450078, 1.9465878, 2.4525469, 3.0900155, 5.0])
@pytest.mark.parametrize("shape", [(61, 97), (480, 640), (7, 5)])
def test_gaussian_blur_bit_exact(ctx, oracle, sigma, shape):
    rng = np.random.default_rng(1)
    img = rng.random(shape, dtype=np.float32)
    assert np.array_equal(ctx.gaussian_blur(img, sigma), oracle.gaussian_blur(img, sigma))


@pytest.mark.parametrize("src,dst", [((13, 17), (26, 34)), ((213, 320), (426, 640)), ((10, 10), (37, 23)),
                                     ((50, 40), (20, 16))])
def test_resize_bit_exact(ctx, oracle, src, dst):
    rng = np.random.default_rng(2)
    img = rng.random(src, dtype=np.float32)
    h2, w2 = dst
    assert np.array_equal(ctx.resize_linear(img, w2, h2), oracle.resize_linear(img, w2, h2))
    assert np.array_equal(ctx.resize_nearest(img, w2, h2), oracle.resize_nearest(img, w2, h2))


def test_compute_descriptor(ctx, oracle):
    """benches/descriptor.rs: (100, 100), scale 2.1, 123 deg on bird.jpg / 255."""
    from conftest import load_golden
    img = load_golden("bird")["image"].astype(np.float32) / 255.0
    rng = np.random.default_rng(3)
    cases = [(100.0, 100.0, 2.1, 123.0)] + [
        (float(rng.uniform(0, 799)), float(rng.uniform(0, 533)), float(rng.uniform(1.8, 3.6)),
         float(rng.uniform(0, 360))) for _ in range(40)]
    same = 0
    for x, y, s, a in cases:
        g = ctx.compute_descriptor(img, x, y, s, a)
        o = oracle.compute_descriptor(img, x, y, s, a)
        d = np.abs(g.astype(int) - o.astype(int))
        assert d.max() <= 1, (x, y, s, a, d.max())
        same += (d == 0).sum()
    assert same == 128 * len(cases)  # sift_mi_compute_descriptor uses the exact accumulation order


def _descriptor_images():
    import patterns
    rng = np.random.default_rng(4)
    return {
        "random_61x97": rng.random((61, 97), dtype=np.float32),
        "checker8": (patterns.make("checker8") // 255).astype(np.float32),
        "constant": np.full((61, 97), 0.3, np.float32),
        "5x7": rng.random((5, 7), dtype=np.float32),
        "3x3": rng.random((3, 3), dtype=np.float32),
        "1x1": rng.random((1, 1), dtype=np.float32),
    }


DESC_IMAGES = _descriptor_images()


@pytest.mark.parametrize("name", list(DESC_IMAGES))
def test_compute_descriptor_domain_edges(ctx, oracle, name):
    """compute_descriptor (src/lib.rs:785-990) at the edges of its domain,
    byte-identical to the oracle (this entry uses the exact accumulation
    order): positions on the corners, outside the image on every side, on the
    rounding tie of the row (y = 0.49 / 0.5) and far away (1e4: saturating
    casts); the smallest window (scale 0.05, radius 1) and the largest the
    host accepts (3.69, radius 39); orientations on the bin boundaries and at
    360; images down to one pixel, whose windows hold no sample at all."""
    img = DESC_IMAGES[name]
    h, w = img.shape
    positions = [(0.0, 0.0), (w - 1.0, h - 1.0), (-3.5, 10.0), (w + 4.0, h + 4.0), (w / 2, 0.49), (w / 2, 0.5),
                 (1e4, 1e4)]
    nonzero = 0
    for x, y in positions:
        for scale in (0.05, 3.69):
            for angle in (0.0, 45.0, 90.0, 360.0):
                g = ctx.compute_descriptor(img, x, y, scale, angle)
                o = oracle.compute_descriptor(img, x, y, scale, angle)
                assert np.array_equal(g, o), (x, y, scale, angle, np.flatnonzero(g != o)[:8])
                if name in ("constant", "1x1") or x == 1e4:
                    assert not g.any(), (x, y, scale, angle)  # no gradient / no sample: 128 zeros
                nonzero += int(g.any())
    if name in ("random_61x97", "checker8", "5x7", "3x3"):
        assert nonzero > 0  # the cases are not all empty windows


def test_compute_descriptor_rejects(pkg, ctx):
    """sift_mi_compute_descriptor refuses, before anything is launched, a
    window radius above its scratch (scale 3.8; scale 0) with
    SIFT_MI_EUNSUPPORTED and an orientation outside [0, 360] (the reference
    indexes out of bounds there) with SIFT_MI_EINVAL; the output buffer is not
    touched."""
    img = DESC_IMAGES["random_61x97"]
    out = np.full(128, 0xA5, np.uint8)

    def rc(scale, angle):
        return pkg.lib().sift_mi_compute_descriptor(ctx._h, img.ctypes.data, img.shape[1], img.shape[0], 30.0, 30.0,
                                                    scale, angle, out.ctypes.data)
    EINVAL, EUNSUPPORTED = -1, -5
    assert rc(3.8, 10.0) == EUNSUPPORTED
    assert rc(0.0, 10.0) == EUNSUPPORTED
    assert rc(2.0, -1.0) == EINVAL
    assert rc(2.0, 360.5) == EINVAL
    assert rc(2.0, float("nan")) == EINVAL
    assert np.all(out == 0xA5)
    assert rc(3.69, 360.0) == 0 and rc(0.05, 0.0) == 0  # the accepted ends of both ranges
