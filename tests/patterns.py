"""Structured u8 test images: exact ties, plateaus and dense keypoints.

The photographs, synth.frame and white noise contain no exact tie: after the
blurs every DoG value, histogram bin and response is a distinct float, so no
branch whose result depends on *equality* is exercised by them (DESIGN.md,
"Structured patterns").  The generators here are pure numpy, deterministic and
keyed by name; shapes are H x W.  The random ones draw u8 directly
(integers(..., dtype=np.uint8): the draw depends on the dtype).  Widths are
>= 80 so the strip seed runs, 161 and 200 give partial strips, heights 97 and
168 odd octave sizes.

A helper module (imported by test_patterns_cpu.py, test_gpu_patterns.py and
test_gpu_ops.py), not a conftest.
"""
import numpy as np


def _grid(h, w):
    y, x = np.mgrid[:h, :w]
    return y, x


def checker(h, w, p):
    y, x = _grid(h, w)
    return ((((y // p) + (x // p)) & 1) * 255).astype(np.uint8)


def squares(h, w, period=16, side=7):
    y, x = _grid(h, w)
    return np.where((y % period < side) & (x % period < side), 255, 0).astype(np.uint8)


def diamonds(h, w):
    y, x = _grid(h, w)
    return np.where(np.abs(x % 16 - 8) + np.abs(y % 16 - 8) < 5, 255, 0).astype(np.uint8)


def diag(h, w, p):
    y, x = _grid(h, w)
    return ((((x + y) // p) & 1) * 255).astype(np.uint8)


def rings(h, w):
    y, x = _grid(h, w)
    r = np.hypot(y - (h - 1) / 2, x - (w - 1) / 2)
    return np.round(127.5 + 127.5 * np.cos(0.45 * r)).astype(np.uint8)


def blocks(h, w, b):
    cells = np.random.default_rng(3).integers(0, 2, (h // b + 1, w // b + 1), dtype=np.uint8) * 255
    return np.kron(cells, np.ones((b, b), np.uint8))[:h, :w].astype(np.uint8)


def tiled32(h, w):
    patch = np.kron(np.random.default_rng(1).integers(0, 256, (8, 8), dtype=np.uint8), np.ones((4, 4), np.uint8))
    return np.tile(patch, (h // 32 + 1, w // 32 + 1))[:h, :w].astype(np.uint8)


def sym4(h, w):
    q = np.kron(np.random.default_rng(2).integers(0, 256, (h // 8, w // 8), dtype=np.uint8), np.ones((4, 4), np.uint8))
    top = np.concatenate([q, q[:, ::-1]], axis=1)
    return np.concatenate([top, top[::-1]], axis=0).astype(np.uint8)


def satblobs(h, w):
    y, x = _grid(h, w)
    return np.clip(np.round(128 + 400 * np.sin(0.21 * x) * np.sin(0.17 * y)), 0, 255).astype(np.uint8)


def bigsq(h, w):
    a = np.zeros((h, w), np.uint8)
    a[30:62, 50:110] = 255
    return a


def flat(h, w, v):
    return np.full((h, w), v, np.uint8)


def step(h, w):
    a = np.zeros((h, w), np.uint8)
    a[:, w // 2:] = 255
    return a


def stars_inv(h, w):
    rng = np.random.default_rng(1)
    ys = rng.integers(0, h, 40)
    xs = rng.integers(0, w, 40)
    a = np.full((h, w), 255, np.uint8)
    a[ys, xs] = 0
    return a


def edge_dots(h, w):
    """3x3 blocks of 255 (clipped at the image edge) at the four corners, the
    four edge midpoints and (2, 2), (h - 3, w - 3)."""
    a = np.zeros((h, w), np.uint8)
    centres = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0),
               (h // 2, w - 1), (2, 2), (h - 3, w - 3)]
    for cy, cx in centres:
        a[max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2] = 255
    return a


def box_noise(h, w, seed, k, gain):
    """u8 noise under a k x k box filter, its contrast stretched by `gain`
    about mid-grey: integer arithmetic throughout."""
    n = np.random.default_rng(seed).integers(0, 256, (h + k - 1, w + k - 1), dtype=np.uint8).astype(np.int64)
    c = np.zeros((h + k, w + k), np.int64)
    c[1:, 1:] = n.cumsum(0).cumsum(1)
    s = c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]
    return np.clip(128 + ((2 * s - 255 * k * k) * gain) // (2 * k * k), 0, 255).astype(np.uint8)


def kron_noise(h, w, seed, b):
    """u8 noise in b x b blocks."""
    c = np.random.default_rng(seed).integers(0, 256, (h // b + 1, w // b + 1), dtype=np.uint8)
    return np.kron(c, np.ones((b, b), np.uint8))[:h, :w].astype(np.uint8)


def streaks(h, w, seed):
    """Elongated quartic bumps (aspect 2-3.5, slope between 1/2 and 2 either
    way) on mid-grey: one about every 8 px along each border, 0.5-5 px inside
    it, and 40 in the interior.  Elongated extrema are the ill-conditioned
    ones: a cross term of the Hessian can carry the Newton offset of one
    coordinate past 0.5 although the pixel is the discrete extremum.  Only
    + - * / and floor: no libm call decides a pixel."""
    rng = np.random.default_rng(seed)
    y, x = _grid(h, w)
    a = np.full((h, w), 128.0)
    cs = []
    for side in range(4):
        length = w if side < 2 else h
        n = length // 8
        t = (np.arange(n) + 0.5) * 8 + rng.uniform(-3, 3, n)
        d = rng.uniform(0.5, 5.0, n)
        for ti, di in zip(t, d):
            cs.append([(di, ti), (h - 1 - di, ti), (ti, di), (ti, w - 1 - di)][side])
    for _ in range(40):
        cs.append((rng.uniform(8, h - 8), rng.uniform(8, w - 8)))
    for cy, cx in cs:
        b = rng.uniform(1.2, 3.0)
        asp = rng.uniform(2.0, 3.5)
        m = rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0)
        nrm2 = 1.0 + m * m
        amp = rng.choice([-1.0, 1.0]) * rng.uniform(50, 127)
        u = (x - cx) + m * (y - cy)
        v = m * (x - cx) - (y - cy)
        q = np.maximum(0.0, 1.0 - (u * u / (asp * asp * b * b) + v * v / (b * b)) / nrm2)
        a += amp * q * q
    return np.clip(np.floor(a + 0.5), 0, 255).astype(np.uint8)


# the kinds of frame a mosaic cell is cut from
MOSAIC_SOURCES = [("box", 3, 2), ("box", 5, 3), ("box", 7, 4), ("kron", 2), ("kron", 3), ("kron", 4), ("streaks",)]
MOSAIC_CELL = 32


def mosaic(h, w, cells):
    """cells[i][j] = (kind, seed): the 32 x 32 cell (i, j) is cut, in place,
    from the h x w frame of MOSAIC_SOURCES[kind] with that seed; the last
    row and column of cells take the remainder of the frame.
    Every cell is a window of a WHOLE source frame: its pixels depend on that
    frame's full random stream, so generating only the window would give
    another image (test_patterns_cpu.COUNTS would notice).  A dozen whole
    frames per mosaic is affordable because make() builds each pattern once."""
    a = np.zeros((h, w), np.uint8)
    ny, nx = len(cells), len(cells[0])
    for i in range(ny):
        for j in range(nx):
            kind, seed = cells[i][j]
            src = MOSAIC_SOURCES[kind]
            full = (box_noise(h, w, seed, src[1], src[2]) if src[0] == "box"
                    else kron_noise(h, w, seed, src[1]) if src[0] == "kron" else streaks(h, w, seed))
            y0, y1 = i * MOSAIC_CELL, (h if i == ny - 1 else (i + 1) * MOSAIC_CELL)
            x0, x1 = j * MOSAIC_CELL, (w if j == nx - 1 else (j + 1) * MOSAIC_CELL)
            a[y0:y1, x0:x1] = full[y0:y1, x0:x1]
    return a


# The refinement fixtures (tests/test_refine_variants_cpu.py).  The decisions
# of interpolate_extremum that they exist for are rare: a Newton move that ends
# exactly one column or row past a border, a refinement that converges on its
# fifth evaluation or gives up after it.  A white-noise or blob frame has a
# fraction of one such keypoint, so the cells below were FOUND, not designed:
# a CPU search (coordinate ascent: for one cell at a time, draw 24-40 random
# (kind, seed) pairs, run the oracle and its wrong-on-purpose variants on the
# whole mosaic in both profiles, keep the pair that raises the number of
# extremum records the variants change; a few sweeps over the cells).  The
# generators need only these constants.
BORDER_MOSAIC_CELLS = [
    [(2, 1771), (5, 428), (3, 1101), (4, 5400), (5, 6219)],
    [(5, 3893), (3, 464), (3, 7090), (4, 34), (5, 7815)],
    [(3, 2100), (4, 8959), (4, 2050), (5, 2371), (5, 4896)],
]
DRIFT_MOSAIC_CELLS = [
    [(5, 1524), (4, 7672), (4, 8031), (4, 7550)],
    [(2, 1888), (2, 2839), (0, 5199), (6, 5349)],
    [(4, 1298), (6, 34), (5, 7297), (5, 4765)],
]


# name -> (H, W, generator(h, w))
REGISTRY = {
    "checker5": (96, 128, lambda h, w: checker(h, w, 5)),
    "checker8": (96, 128, lambda h, w: checker(h, w, 8)),
    "squares": (97, 161, squares),
    # even-sided squares: the tie pattern of the imageproc profile (its DoG
    # extrema sit between two pixels, so two neighbours hold the same value)
    "squares12": (96, 128, lambda h, w: squares(h, w, 12, 8)),
    "diamonds": (96, 128, diamonds),
    "diag7": (96, 128, lambda h, w: diag(h, w, 7)),
    "rings": (96, 128, rings),
    "blocks4": (96, 128, lambda h, w: blocks(h, w, 4)),
    "blocks6": (97, 161, lambda h, w: blocks(h, w, 6)),
    "tiled32": (168, 200, tiled32),
    "sym4": (96, 128, sym4),
    "satblobs": (96, 128, satblobs),
    "bigsq": (97, 161, bigsq),
    "white": (97, 161, lambda h, w: flat(h, w, 255)),
    "step": (97, 161, step),
    "stars_inv": (97, 161, stars_inv),
    "edge_dots": (97, 161, edge_dots),
    # 96 x 128 forms of two of the above and a mid-grey frame, for batches of
    # equal-sized frames (test_pattern_batch_mixed)
    "white_96x128": (96, 128, lambda h, w: flat(h, w, 255)),
    "step_96x128": (96, 128, step),
    "flat77_96x128": (96, 128, lambda h, w: flat(h, w, 77)),
    # the refinement fixtures: Newton moves onto the four border lines, and
    # refinements that take all five evaluations
    "border_mosaic": (97, 161, lambda h, w: mosaic(h, w, BORDER_MOSAIC_CELLS)),
    "drift_mosaic": (96, 128, lambda h, w: mosaic(h, w, DRIFT_MOSAIC_CELLS)),
    # seed 13 of 80 streak frames tried: in the OpenCV profile three
    # refinements converge on a sixth evaluation (which the reference never
    # makes) and three moves have a half-integer offset (roundf against rintf)
    "streaks13": (96, 128, lambda h, w: streaks(h, w, 13)),
}

# the patterns that yield no keypoint in either profile
ZERO_KEYPOINTS = ("white", "step", "stars_inv", "white_96x128", "step_96x128", "flat77_96x128")

_cache = {}


def make(name):
    """The named pattern as a read-only (H, W) u8 array (built once)."""
    if name not in _cache:
        h, w, gen = REGISTRY[name]
        a = np.ascontiguousarray(gen(h, w), dtype=np.uint8)
        assert a.shape == (h, w), (name, a.shape)
        a.setflags(write=False)
        _cache[name] = a
    return _cache[name]


def names():
    return list(REGISTRY)


def response_groups(responses):
    """Groups of bit-equal responses in the descending stable order (the order
    features_limit cuts): a list of (a, b) half-open position ranges with
    b - a >= 2, and the permutation that gives the order."""
    r = np.asarray(responses, np.float32)
    order = np.argsort(-r, kind="stable")
    s = r[order]
    cuts = np.flatnonzero(np.diff(s) != 0) + 1
    starts = np.concatenate([[0], cuts])
    ends = np.concatenate([cuts, [len(s)]])
    return [(int(a), int(b)) for a, b in zip(starts, ends) if b - a >= 2], order
