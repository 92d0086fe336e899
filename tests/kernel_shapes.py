"""Frame shapes on the dispatch thresholds of the pyramid and detection
kernels, and a Python mirror of the integer arithmetic that picks a kernel.

pyramid.hip and scan.hip choose a kernel family per octave by hard thresholds
on the octave's width W and height H.  CASES holds one entry per input shape
that puts an octave on such a threshold (or one step to either side of it):

  * capacity / partner: k_octave_tail's first octave at its LDS limit
    (tail_octave_start, pyramid.hip:2231: tail_lds_floats + 4 W + 64 <=
    kTailLdsFloats = 39680; the slack covers the last row / column items'
    reads of up to 3 rows / columns past a halo, pyramid.hip:2009), and the
    shape one pixel wider, which is over the limit and starts the tail one
    octave later;
  * seed: the strip seed and the seed pair, seed W >= 160 && H >= 64
    (pyramid.hip:1865, :1909);
  * pair: the pair blur, W >= 64 && H >= 64 (pyramid.hip:1784);
  * strip: the strip blur against the tile blur, W > R && H > R
    (pyramid.hip:1808), at W or H of R and R + 1 for every radius;
  * seam: octaves one strip wide, one strip less or plus one column (128
    columns, StripGeom; 112 / 120 output columns of the OpenCV / imageproc
    pair strips, PairGeom::TWO);
  * fused: the fused blur-5 + extremum scan, W > R + 1 && H > R + 1
    (scan.hip:751), its 62- / 124-column waves (DR_COLS, BD2_COLS) and the
    32-row segments of path option fused_detect = 2;
  * rows: octave heights around one or two strip_segment_rows segments and the
    32-row chunk.

The mirror restates, in integers only:
  octave sizes   (2w >> o, 2h >> o), o < n_octaves (geometry.cpp);
  tail_pa, tail_tp, tail_lds_floats, tail_octave_start (pyramid.hip:1975-2234);
  the pyramid_launches of one precompute_images call (PyramidRun,
  pipeline.cpp:427-602).

Launch rule (stats()["pyramid_launches"] after one precompute_images):
  1 for the seed, whether it is k_seed / k_seed_strip or k_seed_pair (which
  also writes G_1 of octave 0);
  per octave below the first tail octave, one per blur launch, a pair launch
  counting once:
      octave 0, seed pair and the (2, 3) pair apply      3  (pair, 4, 5)
      octave 0, seed pair without the (2, 3) pair        4  (single octave)
      octave 0, only the (1, 2) pair applies             4
      octave 0, neither                                  5
      octave >= 1, the (1, 2) pair applies               4
      octave >= 1, it does not                           5
  1 more when a tail octave exists (k_octave_tail, every tail octave in one
  launch).  The DoG launches (k_dog) are not counted.  The seed pair needs
  seed W >= 160 && H >= 64 and the path options pair_blur, seed_pair; a pair
  needs W >= 64 && H >= 64 and pair_blur; tile_blur = 1 turns both off.

Each case carries the literal first tail octave and launch count per profile
under its primary path options (EXPECT).  tests/test_kernel_shapes_cpu.py
checks the literals against the mirror and the mirror's claims (capacity,
sides of each predicate, keypoints near each seam) against the CPU oracle;
tests/test_gpu_thresholds.py asserts the launch counts on the device, which
pins the mirror to the library.

A helper module, not a conftest.
"""
import collections
import math

import numpy as np

import patterns

OPENCV, IMAGEPROC = 0, 1
PROFILES = (OPENCV, IMAGEPROC)

K_IMAGES_PER_OCTAVE = 6
K_TAIL_LDS_FLOATS = 39680  # sift_kernels.h kTailLdsFloats
K_TAIL_MAX_OCT = 16        # sift_kernels.h kTailMaxOct
K_IMAGE_BORDER = 5         # sift_common.h kImageBorder
# radii of blurs 1..5 of an octave (index 0 unused), pyramid.hip:2131
OCT_R = {OPENCV: (0, 5, 6, 8, 10, 13), IMAGEPROC: (0, 3, 4, 4, 5, 7)}
STRIP_TW = 128                             # StripGeom::TW
PAIR_TWO = {OPENCV: 112, IMAGEPROC: 120}   # PairGeom::TWO = 128 - 2 HB
DR_COLS, BD2_COLS = 62, 124                # scan.hip

# path-option sets by name (Context.path_options keywords)
OPTION_SETS = {
    "default": {},
    "notail": {"tail": 0},
    "nopair": {"pair_blur": 0},
    "noseedpair": {"seed_pair": 0},
    "single": {"pair_blur": 0, "tail": 0},
}


# ---------------------------------------------------------------------------
# the mirror
# ---------------------------------------------------------------------------
def n_octaves(w, h):
    """round(log2(min(2w, 2h)) - 2) as usize + 1 (geometry.cpp n_octaves_for;
    roundf rounds halves away from zero, the cast saturates at 0)."""
    f = math.log2(min(2 * w, 2 * h)) - 2.0
    r = math.floor(f + 0.5) if f >= 0 else -math.floor(-f + 0.5)
    return max(int(r), 0) + 1


def octave_sizes(w, h):
    return [((2 * w) >> o, (2 * h) >> o) for o in range(n_octaves(w, h))]


def tail_pa(W, rm):
    return (W + 2 * rm) | 1


def tail_tp(W):
    return W | 1


def tail_lds_floats(W, H, rm):
    return 2 * tail_pa(W, rm) * H + tail_tp(W) * (H + 2 * rm) + (W // 2) * (H // 2)


def tail_use(W, H, profile):
    """What tail_octave_start compares with kTailLdsFloats: the layout plus
    the slack for the reads past the halos."""
    return tail_lds_floats(W, H, max(OCT_R[profile])) + 4 * W + 64


def tail_octave_start(sizes, profile, tail=1):
    n = len(sizes)
    if not tail or n > K_TAIL_MAX_OCT:
        return n
    for o, (W, H) in enumerate(sizes):
        next_ok = o + 1 >= n or sizes[o + 1][0] * sizes[o + 1][1] <= 4096
        if tail_use(W, H, profile) <= K_TAIL_LDS_FLOATS and next_ok:
            return o
    return n


def seed_pair_applies(W0, H0, opts=None):
    o = dict(opts or {})
    return bool(W0 >= 160 and H0 >= 64 and o.get("pair_blur", 1) and o.get("seed_pair", 1)
                and not o.get("tile_blur", 0))


def pair_applies(W, H, opts=None):
    o = dict(opts or {})
    return bool(W >= 64 and H >= 64 and o.get("pair_blur", 1) and not o.get("tile_blur", 0))


def strip_applies(W, H, R, opts=None):
    return bool(W > R and H > R and not dict(opts or {}).get("tile_blur", 0))


def strip_segments(rows, per, target=6144):
    """Row segments of a strip launch over `rows` rows with `per` strips x
    frames (strip_segment_rows, pyramid.hip:1716): (segment length, count)."""
    few = min((2048 + per - 1) // per, rows // 40)
    nseg = max(1, min((target + per - 1) // per, max(rows // 320, few)))
    seg = ((rows + nseg - 1) // nseg + 1) & ~1
    return seg, (rows + seg - 1) // seg


def fused_applies(W, H, profile, opts=None):
    """blur_detect_segment > 0 for one frame of a test-sized octave: only under
    fused_detect = 2 (the default, 1, wants >= 8192 waves per launch)."""
    R = OCT_R[profile][5]
    return bool(dict(opts or {}).get("fused_detect", 1) == 2 and W > R + 1 and H > R + 1
                and W >= 2 * K_IMAGE_BORDER and H >= 2 * K_IMAGE_BORDER)


def dispatch(w, h, profile, opts=None):
    """(first tail octave, pyramid_launches) of one precompute_images."""
    o_ = dict(opts or {})
    sizes = octave_sizes(w, h)
    n = len(sizes)
    o_tail = tail_octave_start(sizes, profile, o_.get("tail", 1))
    launches = 1
    seed_pair = seed_pair_applies(*sizes[0], o_)
    for o in range(o_tail):
        pair = pair_applies(*sizes[o], o_)
        if o == 0 and seed_pair:
            # the (2, 3) pair writes the next octave's base: it needs one
            launches += 3 if pair and n > 1 else 4
        else:
            launches += 4 if pair else 5
    if o_tail < n:
        launches += 1
    return o_tail, launches


def fused_octaves(w, h, profile, opts=None):
    """The octaves whose blur 5 and extremum scan run as one pass in a
    one-frame sift() call: those below the tail where the pass applies."""
    sizes = octave_sizes(w, h)
    o_tail = tail_octave_start(sizes, profile, dict(opts or {}).get("tail", 1))
    return [o for o in range(min(o_tail, 32)) if fused_applies(*sizes[o], profile, opts)]


def blur_families(w, h, profile, opts=None):
    """[(octave, blur, R, W, H, 'strip' | 'tile')] of the single-blur launches
    below the tail (pair launches left out)."""
    o_ = dict(opts or {})
    sizes = octave_sizes(w, h)
    o_tail = tail_octave_start(sizes, profile, o_.get("tail", 1))
    seed_pair = seed_pair_applies(*sizes[0], o_)
    out = []
    for o in range(o_tail):
        W, H = sizes[o]
        pair = pair_applies(W, H, o_)
        first = 1
        if o == 0 and seed_pair:
            first = 4 if pair and len(sizes) > 1 else 2
        elif pair:
            first = 3
        for s in range(first, K_IMAGES_PER_OCTAVE):
            R = OCT_R[profile][s]
            out.append((o, s, R, W, H, "strip" if strip_applies(W, H, R, o_) else "tile"))
    return out


# ---------------------------------------------------------------------------
# images
# ---------------------------------------------------------------------------
def noise(w, h):
    """Seeded uniform u8 noise: every neighbour differs, so a shifted,
    duplicated or stale row or column of a plane cannot cancel."""
    return np.random.default_rng(1000 * w + h).integers(0, 256, (h, w), dtype=np.uint8)


def seam_shift(seam):
    """Columns to shift the 12-px square lattice left so that a column of its
    extrema falls on the seam (the lattice's extrema sit at x = 8 mod 24 in
    octave 0 and x = 4 mod 12 in octave 1)."""
    if seam is None:
        return 0
    o, c = seam
    return ((8 - c) % 24) // 2 if o == 0 else (4 - c) % 12


def pattern_images(case):
    """name -> u8 image of the case's keypoint inputs: patterns.blocks(h, w, 4)
    and patterns.squares(h, w, 12, 8), the latter phase-shifted onto the
    case's seam; frames under 16 px on a side, where the 12-px lattice has no
    extremum inside the 5-px border, add patterns.squares(h, w, 5, 3)."""
    w, h, sh = case.w, case.h, seam_shift(case.seam)
    out = {"blocks4": patterns.blocks(h, w, 4),
           "squares12": np.ascontiguousarray(patterns.squares(h, w + sh, 12, 8)[:, sh:])}
    if min(w, h) < 16:
        out["squares5"] = patterns.squares(h, w, 5, 3)
    return out


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------
# name: "<kind>_<w>x<h>"; opts: the primary option set (EXPECT's literals are
# for it); also: further option sets to run (their counts come from the
# mirror); target: file:line and a sentence; pred: (predicate, octave) the case
# straddles and holds: its value per profile (None: not aimed at that
# profile); group: the cases that together sit on both sides of it; cap: the
# profile whose tail is at capacity, partner: the capacity case this one is
# one pixel wider than; seam: (octave, column) of the strip / wave boundary
# and seam_profiles: where that family runs; detect: run the keypoint stages.
Case = collections.namedtuple(
    "Case", "name kind w h opts also target why pred holds group cap partner seam seam_profiles detect tail launches")

# (first tail octave, pyramid_launches) per profile (OpenCV, imageproc) under
# the case's primary options
EXPECT = {
    "capacity_48x50": ((0, 2), (0, 2)),
    "partner_49x50": ((1, 6), (0, 2)),
    "capacity_96x100": ((1, 5), (1, 5)),
    "capacity_97x100": ((1, 5), (1, 5)),
    "partner_98x100": ((2, 9), (1, 5)),
    "capacity_32x243": ((1, 6), (1, 6)),
    "partner_33x243": ((2, 11), (1, 6)),
    "capacity_155x63": ((1, 5), (1, 5)),
    "partner_156x63": ((2, 10), (1, 5)),
    "capacity_473x16": ((1, 7), (1, 7)),
    "partner_474x16": ((2, 12), (1, 7)),
    "capacity_236x8": ((0, 2), (0, 2)),
    "partner_237x8": ((1, 7), (0, 2)),
    "capacity_11x449": ((1, 7), (1, 7)),
    "partner_12x449": ((2, 12), (1, 7)),
    "capacity_25x100": ((1, 7), (0, 2)),
    "partner_26x100": ((1, 7), (1, 7)),
    "capacity_98x27": ((1, 7), (0, 2)),
    "partner_99x27": ((1, 7), (1, 7)),
    "capacity_75x141": ((2, 10), (1, 6)),
    "partner_76x141": ((2, 10), (2, 10)),
    "capacity_120x89": ((2, 9), (1, 5)),
    "partner_121x89": ((2, 9), (2, 9)),
    "capacity_196x54": ((2, 10), (1, 5)),
    "partner_197x54": ((2, 10), (2, 10)),
    "capacity_327x31": ((2, 12), (1, 7)),
    "partner_328x31": ((2, 12), (2, 12)),
    "capacity_9x692": ((2, 12), (1, 7)),
    "partner_10x692": ((2, 12), (2, 12)),
    "seed_79x40": ((1, 6), (1, 6)),
    "seed_80x40": ((1, 5), (1, 5)),
    "seed_81x40": ((1, 5), (1, 5)),
    "seed_80x31": ((1, 7), (0, 2)),
    "seed_80x32": ((1, 5), (0, 2)),
    "seed_80x33": ((1, 5), (0, 2)),
    "seed_79x32": ((1, 6), (0, 2)),
    "pair_63x400": ((2, 11), (2, 11)),
    "pair_64x400": ((2, 10), (2, 10)),
    "pair_65x400": ((2, 10), (2, 10)),
    "pair_400x63": ((2, 10), (2, 10)),
    "pair_400x64": ((2, 9), (2, 9)),
    "pair_63x64": ((6, 30), (6, 30)),
    "pair_64x63": ((6, 30), (6, 30)),
    "pair_64x64": ((6, 29), (6, 29)),
    "strip_28x28": ((5, 26), (5, 26)),
    "strip_26x26": ((5, 26), (5, 26)),
    "strip_22x22": ((4, 21), (4, 21)),
    "strip_20x20": ((4, 21), (4, 21)),
    "strip_18x18": ((4, 21), (4, 21)),
    "strip_16x16": ((4, 21), (4, 21)),
    "strip_14x14": ((4, 21), (4, 21)),
    "strip_13x40": ((4, 21), (4, 21)),
    "strip_14x40": ((4, 21), (4, 21)),
    "strip_15x40": ((4, 21), (4, 21)),
    "strip_16x40": ((4, 21), (4, 21)),
    "strip_40x13": ((4, 21), (4, 21)),
    "strip_40x14": ((4, 21), (4, 21)),
    "strip_40x15": ((4, 21), (4, 21)),
    "strip_40x16": ((4, 21), (4, 21)),
    "strip_8x40": ((3, 16), (3, 16)),
    "strip_9x40": ((3, 16), (3, 16)),
    "strip_40x8": ((3, 16), (3, 16)),
    "seam_127x40": ((1, 5), (1, 5)),
    "seam_128x40": ((1, 5), (1, 5)),
    "seam_129x40": ((1, 5), (1, 5)),
    "seam_257x40": ((2, 10), (1, 5)),
    "seam_111x40": ((1, 5), (1, 5)),
    "seam_112x40": ((1, 5), (1, 5)),
    "seam_113x40": ((1, 5), (1, 5)),
    "seam_224x40": ((1, 5), (1, 5)),
    "seam_225x40": ((1, 5), (1, 5)),
    "seam_119x40": ((1, 5), (1, 5)),
    "seam_120x40": ((1, 5), (1, 5)),
    "seam_121x40": ((1, 5), (1, 5)),
    "seam_240x40": ((2, 10), (1, 5)),
    "seam_127x64": ((1, 5), (1, 5)),
    "seam_128x64": ((1, 5), (1, 5)),
    "seam_129x64": ((1, 5), (1, 5)),
    "seam_257x64": ((2, 9), (2, 9)),
    "seam_111x64": ((1, 5), (1, 5)),
    "seam_112x64": ((1, 5), (1, 5)),
    "seam_113x64": ((1, 5), (1, 5)),
    "seam_224x64": ((2, 9), (2, 9)),
    "seam_225x64": ((2, 9), (2, 9)),
    "seam_119x64": ((1, 5), (1, 5)),
    "seam_120x64": ((1, 5), (1, 5)),
    "seam_121x64": ((1, 5), (1, 5)),
    "seam_240x64": ((2, 9), (2, 9)),
    "fused_61x31": ((0, 2), (0, 2)),
    "fused_61x32": ((0, 2), (0, 2)),
    "fused_61x33": ((0, 2), (0, 2)),
    "fused_61x48": ((1, 6), (1, 6)),
    "fused_62x31": ((0, 2), (0, 2)),
    "fused_62x32": ((0, 2), (0, 2)),
    "fused_62x33": ((0, 2), (0, 2)),
    "fused_62x48": ((1, 6), (1, 6)),
    "fused_63x31": ((0, 2), (0, 2)),
    "fused_63x32": ((0, 2), (0, 2)),
    "fused_63x33": ((0, 2), (0, 2)),
    "fused_63x48": ((1, 6), (1, 6)),
    "fused_123x31": ((1, 7), (1, 7)),
    "fused_123x32": ((1, 5), (1, 5)),
    "fused_123x33": ((1, 5), (1, 5)),
    "fused_123x48": ((1, 5), (1, 5)),
    "fused_124x31": ((1, 7), (1, 7)),
    "fused_124x32": ((1, 5), (1, 5)),
    "fused_124x33": ((1, 5), (1, 5)),
    "fused_124x48": ((1, 5), (1, 5)),
    "fused_125x31": ((1, 7), (1, 7)),
    "fused_125x32": ((1, 5), (1, 5)),
    "fused_125x33": ((1, 5), (1, 5)),
    "fused_125x48": ((1, 5), (1, 5)),
    "fused_248x31": ((1, 7), (1, 7)),
    "fused_248x32": ((1, 5), (1, 5)),
    "fused_248x33": ((1, 5), (1, 5)),
    "fused_248x48": ((2, 10), (2, 10)),
    "fusedr_14x40": ((4, 21), (4, 21)),
    "fusedr_40x14": ((4, 21), (4, 21)),
    "fusedr_15x40": ((4, 21), (4, 21)),
    "fusedr_16x40": ((4, 21), (4, 21)),
    "fusedr_40x15": ((4, 21), (4, 21)),
    "rows_97x39": ((1, 5), (1, 5)),
    "rows_97x40": ((1, 5), (1, 5)),
    "rows_97x41": ((1, 5), (1, 5)),
    "rows_97x79": ((1, 5), (1, 5)),
    "rows_97x80": ((1, 5), (1, 5)),
    "rows_97x81": ((1, 5), (1, 5)),
}

CASES = []


def _add(kind, w, h, opts, also, target, why, pred=None, holds=(None, None), group=None, cap=None, partner=None,
         seam=None, seam_profiles=PROFILES, detect=False):
    name = f"{kind}_{w}x{h}"
    t, l = zip(*EXPECT[name])
    CASES.append(Case(name, kind, w, h, opts, tuple(also), target, why, pred, tuple(holds), group, cap, partner, seam,
                      tuple(seam_profiles), detect, tuple(t), tuple(l)))


def _wh(s):
    return tuple(map(int, s.split("x")))


CAPACITY = {OPENCV: ["48x50", "96x100", "97x100", "32x243", "155x63", "473x16", "236x8", "11x449"],
            IMAGEPROC: ["25x100", "98x27", "75x141", "120x89", "196x54", "327x31", "9x692"]}


def _build():
    T = "pyramid.hip:2231"
    for p in PROFILES:
        for s in CAPACITY[p]:
            w, h = _wh(s)
            g = s  # the group ends at the first wider frame over the limit (96x100, 97x100 | 98x100)
            while "%dx%d" % (_wh(g)[0] + 1, h) in CAPACITY[p]:
                g = "%dx%d" % (_wh(g)[0] + 1, h)
            _add("capacity", w, h, "default", (), T,
                 "the first tail octave uses 39670-39679 of the 39680 LDS floats: the slack for the reads past "
                 "the halos is all there is", pred=("tail", None), holds=[True if q == p else None for q in PROFILES],
                 group=f"tail_{g}", cap=p, detect=True)
            if f"{w + 1}x{h}" not in CAPACITY[p]:  # (97x100 is itself at capacity)
                _add("partner", w + 1, h, "default", (), T,
                     f"one pixel wider than {s}: over the limit, the tail starts one octave later",
                     pred=("tail", None), holds=[False if q == p else None for q in PROFILES], group=f"tail_{g}",
                     partner=f"capacity_{s}", detect=True)
    for s, hold in [("79x40", False), ("80x40", True), ("81x40", True), ("80x31", False), ("80x32", True),
                    ("80x33", True), ("79x32", False)]:
        w, h = _wh(s)
        _add("seed", w, h, "default", ("notail", "nopair", "noseedpair"), "pyramid.hip:1865, :1909",
             "seed W >= 160 && H >= 64: k_seed_strip / k_seed_pair on one side, the tile seed on the other",
             pred=("seed", 0), holds=(hold, hold), group="seed")
    for s, opt, o, hold in [("63x400", "default", 1, False), ("64x400", "default", 1, True),
                            ("65x400", "default", 1, True), ("400x63", "default", 1, False),
                            ("400x64", "default", 1, True), ("63x64", "notail", 1, False),
                            ("64x63", "notail", 1, False), ("64x64", "notail", 1, True)]:
        w, h = _wh(s)
        _add("pair", w, h, opt, ("notail", "nopair"), "pyramid.hip:1784",
             "W >= 64 && H >= 64 in an octave below the tail: k_blur2_strip on one side, two single blurs on the other",
             pred=("pair", o), holds=(hold, hold), group="pair")
    for s in ["28x28", "26x26", "22x22", "20x20", "18x18", "16x16", "14x14", "13x40", "14x40", "15x40", "16x40", "40x13",
              "40x14", "40x15", "40x16", "8x40", "9x40", "40x8"]:
        w, h = _wh(s)
        _add("strip", w, h, "notail", ("single",), "pyramid.hip:1808",
             "W > R && H > R: an octave of width or height R + 1 takes k_blur_strip with exactly one reflection, "
             "one of R the tile kernel", group="strip")
    for h in (40, 64):
        for w in (127, 128, 129, 257):
            _add("seam", w, h, "default", ("notail", "nopair", "noseedpair", "single"), "pyramid.hip:288 (StripGeom::TW)",
                 "octave 1 is one 128-column strip less a column, exactly one, one plus a column, two plus a column; "
                 "octave 0 has the seam inside", seam=(1, 128) if w == 257 else (0, 128), detect=True)
        for w in (111, 112, 113, 224, 225):
            _add("seam", w, h, "default", ("notail", "nopair", "noseedpair", "single"), "pyramid.hip:694 (PairGeom::TWO)",
                 "the OpenCV pair kernels' 112 output columns per strip: an octave of one or two strips less a "
                 "column, exactly, plus a column",
                 seam=(0, 112) if w < 200 else ((1, 112) if h == 64 else (0, 224)), seam_profiles=(OPENCV,), detect=True)
        for w in (119, 120, 121, 240):
            _add("seam", w, h, "default", ("notail", "nopair", "noseedpair", "single"), "pyramid.hip:694 (PairGeom::TWO)",
                 "the imageproc pair kernels' 120 output columns per strip: an octave of one or two strips less a "
                 "column, exactly, plus a column",
                 seam=(0, 120) if w < 200 else ((1, 120) if h == 64 else (0, 240)), seam_profiles=(IMAGEPROC,),
                 detect=True)
    for w in (61, 62, 63, 123, 124, 125, 248):
        for h in (31, 32, 33, 48):
            _add("fused", w, h, "default", ("notail",), "scan.hip:38, :494 (DR_COLS, BD2_COLS), :757",
                 "octave 1 (width w) and octave 0 (2w) are whole 62- / 124-column waves less a column, exactly, plus "
                 "a column; heights around the 32-row segment",
                 seam=(0, 62) if w < 100 else ((0, 124) if w < 200 else (1, 124)), detect=True)
    for s, hold in [("14x40", (False, None)), ("40x14", (False, None)), ("15x40", (True, True)),
                    ("16x40", (True, True)), ("40x15", (True, True))]:
        w, h = _wh(s)
        _add("fusedr", w, h, "notail", (), "scan.hip:751",
             "W > R + 1 && H > R + 1 in octave 1: width or height 15 is the first the OpenCV fused pass takes (R = 13), "
             "14 goes to launch_blur + k_detect_rows", pred=("fused", 1), holds=hold, group="fused", detect=True)
    for h in (39, 40, 41, 79, 80, 81):
        _add("rows", 97, h, "default", ("notail", "single"), "pyramid.hip:1716 (strip_segment_rows)",
             "octave 0 of 78 / 80 / 82 rows is 1 / 2 / 2 row segments (rows / 40), of 158 / 160 / 162 rows 3 / 4 / 4; "
             "octave 1 one 32-row chunk and a few rows, or two and a half",
             detect=True)


_build()
BY_NAME = {c.name: c for c in CASES}


def predicate(case, profile):
    """The value of the case's predicate under its primary options."""
    name, o = case.pred
    opts = OPTION_SETS[case.opts]
    sizes = octave_sizes(case.w, case.h)
    if name == "tail":
        # the capacity case's first tail octave (the partner: the same octave
        # of the wider frame) is at or under the limit
        ref = BY_NAME[case.partner] if case.partner else case
        o = tail_octave_start(octave_sizes(ref.w, ref.h), profile)
        return tail_use(*sizes[o], profile) <= K_TAIL_LDS_FLOATS
    if name == "seed":
        return seed_pair_applies(*sizes[0], opts)
    if name == "pair":
        return pair_applies(*sizes[o], opts)
    if name == "fused":
        return fused_applies(*sizes[o], profile, {"fused_detect": 2})
    raise KeyError(name)


def pyramid_option_sets(case):
    return (case.opts,) + tuple(a for a in case.also if a != case.opts)


# keypoint runs: path options of the batch path; the fused and seam cases add
# tail = 0, without which their small octaves all go to k_octave_tail and the
# fused pass never sees them
DETECT_MODES = {
    "default": {},
    "apart": {"fused_detect": 0},
    "pair": {"fused_detect": 2, "bd_pair": 1},
    "single": {"fused_detect": 2, "bd_pair": 0},
    "pair_notail": {"fused_detect": 2, "bd_pair": 1, "tail": 0},
    "single_notail": {"fused_detect": 2, "bd_pair": 0, "tail": 0},
    "apart_notail": {"fused_detect": 0, "tail": 0},
}


def detect_modes(case):
    base = ["default", "apart", "pair", "single"]
    if case.kind in ("fused", "fusedr", "seam", "rows"):
        base += ["pair_notail", "single_notail", "apart_notail"]
    return base
