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
