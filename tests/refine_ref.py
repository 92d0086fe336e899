"""A numpy restatement of the oracle's refinement stage (TEST INFRASTRUCTURE).

point_is_local_extremum, interpolate_extremum, extremum_contrast and
extremum_is_on_edge (oracle/sift_oracle.c is_extremum / interpolate /
contrast_at / on_edge) over the DoG planes of `oracle.Pyramid(...).dog(o)`:
f32 scalars, the same expressions in the same order, no variant switch.  It
exists to *describe* a fixture without any wrong variant -- how many Newton
evaluations each candidate took and which rule rejected it -- and is validated
against the oracle (test_refine_variants_cpu.py: the accepted
(octave, s_init, y_init, x_init) sets are equal), not the other way round.

A helper module, not a conftest.
"""
import collections
import math

import numpy as np

BORDER = 5
SCALES = 3
MAX_STEPS = 5
F = np.float32

# why a candidate left the refinement
RULES = ("accept", "x_lo", "x_hi", "y_lo", "y_hi", "s_lo", "s_hi", "steps", "contrast", "edge", "overflow")


def candidates(dog):
    """(s, y, x) of the pixels of one octave's DoG stack (5, h, w) that pass
    point_is_local_extremum, in the oracle's scan order."""
    h, w = dog.shape[1:]
    B = BORDER
    out = []
    if h < 2 * B or w < 2 * B:
        return out
    for s in range(1, SCALES + 1):
        val = dog[s, B:h - B, B:w - B]
        mx = np.full(val.shape, -np.inf, np.float32)
        mn = np.full(val.shape, np.inf, np.float32)
        for ds in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if ds == dy == dx == 0:
                        continue
                    nb = dog[s + ds, B + dy:h - B + dy, B + dx:w - B + dx]
                    mx = np.maximum(mx, nb)
                    mn = np.minimum(mn, nb)
        ys, xs = np.nonzero(((val > 0) & (val >= mx)) | ((val < 0) & (val <= mn)))
        out += [(s, int(y) + B, int(x) + B) for y, x in zip(ys, xs)]
    return out


def _round_away(v):
    """roundf, then the oracle's saturating cast and its limit on the rounded
    move (sat_i64 and LIM = 2^40 in interpolate): None when the move is
    rejected for its size."""
    v = float(v)
    if v != v:
        return 0  # sat_i64(NaN) == 0, Rust's `NaN as isize`
    if math.isinf(v):
        return None  # saturates to +-2^63, beyond the limit
    r = int(math.copysign(math.floor(abs(v) + 0.5), v))  # half away from zero; exact in double for an f32 v
    return None if abs(r) > 2 ** 40 else r


def refine(dog, s, y, x):
    """One candidate through interpolate_extremum and the two tests after it.
    Returns (rules, evaluations, moves, final): `rules` is ("accept",) or the
    rule(s) that rejected it (a move may break several bounds at once),
    `evaluations` the number of Newton systems solved, `moves` the list of
    (ds, dy, dx) taken or attempted, `final` the (s, y, x) of the last
    evaluation."""
    h, w = dog.shape[1:]
    moves = []
    with np.errstate(all="ignore"):
        for it in range(MAX_STEPS):
            n = dog[s - 1:s + 2, y - 1:y + 2, x - 1:x + 2]
            prev, curr, nxt = n[0], n[1], n[2]
            g1 = (nxt[1, 1] - prev[1, 1]) / F(2)
            g2 = (curr[2, 1] - curr[0, 1]) / F(2)
            g3 = (curr[1, 2] - curr[1, 0]) / F(2)
            v2 = curr[1, 1] * F(2)
            h11 = nxt[1, 1] + prev[1, 1] - v2
            h12 = (nxt[2, 1] - nxt[0, 1] - prev[2, 1] + prev[0, 1]) / F(4)
            h13 = (nxt[1, 2] - nxt[1, 0] - prev[1, 2] + prev[1, 0]) / F(4)
            h22 = curr[2, 1] + curr[0, 1] - v2
            h33 = curr[1, 2] + curr[1, 0] - v2
            h23 = (curr[2, 2] - curr[2, 0] - curr[0, 2] + curr[0, 0]) / F(4)
            det = h11 * h22 * h33 - h11 * h23 * h23 - h12 * h12 * h33 + F(2) * h12 * h13 * h23 - h13 * h13 * h22
            i11 = (h22 * h33 - h23 * h23) / det
            i12 = (h13 * h23 - h12 * h33) / det
            i13 = (h12 * h23 - h13 * h22) / det
            i22 = (h11 * h33 - h13 * h13) / det
            i23 = (h12 * h13 - h11 * h23) / det
            i33 = (h11 * h22 - h12 * h12) / det
            os_ = -(i11 * g1 + i12 * g2 + i13 * g3)
            ox = -(i13 * g1 + i23 * g2 + i33 * g3)
            oy = -(i12 * g1 + i22 * g2 + i23 * g3)
            if abs(os_) < F(0.5) and abs(ox) < F(0.5) and abs(oy) < F(0.5):
                interp = os_ * g1 + oy * g2 + ox * g3
                contrast = abs(curr[1, 1] + interp / F(2))
                if contrast * F(SCALES) <= F(0.04):
                    return ("contrast",), it + 1, moves, (s, y, x)
                tr = h33 + h22
                det2 = h33 * h22 - h23 * h23
                if det2 <= F(0) or tr * tr * F(10) > F(121) * det2:
                    return ("edge",), it + 1, moves, (s, y, x)
                return ("accept",), it + 1, moves, (s, y, x)
            r = [_round_away(v) for v in (os_, oy, ox)]
            if None in r:
                return ("overflow",), it + 1, moves, (s, y, x)
            moves.append(tuple(r))
            ns, ny, nx = s + r[0], y + r[1], x + r[2]
            broken = [name for name, bad in (("s_lo", ns < 1), ("s_hi", ns > SCALES), ("x_lo", nx < BORDER),
                                             ("x_hi", nx >= w - BORDER), ("y_lo", ny < BORDER),
                                             ("y_hi", ny >= h - BORDER)) if bad]
            if broken:
                return tuple(broken), it + 1, moves, (s, y, x)
            s, y, x = ns, ny, nx
    return ("steps",), MAX_STEPS, moves, (s, y, x)


def describe(pyramid):
    """The whole refinement stage of an oracle.Pyramid.  Returns a dict:
    accepted   set of (octave, s_init, y_init, x_init)
    rules      Counter over RULES (a candidate counts once per rule it broke)
    accepted_at, decided_at   Counters: evaluations taken -> candidates
    scale_moves  Counter of the sign of every scale move taken or attempted
    records    list of (octave, s, y, x, rules, evaluations, moves, final)"""
    d = dict(accepted=set(), rules=collections.Counter(), accepted_at=collections.Counter(),
             decided_at=collections.Counter(), scale_moves=collections.Counter(), records=[])
    for o in range(pyramid.n_octaves):
        dog = pyramid.dog(o)
        for s, y, x in candidates(dog):
            rules, evals, moves, final = refine(dog, s, y, x)
            d["records"].append((o, s, y, x, rules, evals, moves, final))
            d["rules"].update(rules)
            d["decided_at"][evals] += 1
            d["scale_moves"].update(int(np.sign(m[0])) for m in moves if m[0])
            if rules == ("accept",):
                d["accepted"].add((o, s, y, x))
                d["accepted_at"][evals] += 1
    return d
