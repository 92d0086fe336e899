"""numpy restatement of guided matching -- the segmented 2-NN matcher over the
(query, train) elements a pair's verified model admits -- and the inputs its
tests share (test_guided_ref_cpu.py pins it; test_gpu_match_guided.py holds
the GPU path, csrc/match_guided.hip, against it).  LABELLED EXTENSION: the
crate has nothing like it.

A pair has query keypoints (x_i, y_i), train keypoints (X_j, Y_j), u8
descriptors of both, a model g (9 f32, row-major: the H of verify_ref or the F
of epipolar_ref) and a threshold thr.

    admissible  (i, j) is admissible when the verification's own inlier test
                holds for the record (x_i, y_i, X_j, Y_j): verify_ref.inlier_mask
                for a homography, epipolar_ref.inlier_mask (Sampson) for a
                fundamental matrix.  The predicate is IMPORTED from those two
                modules, never restated, so the gate and the verification's
                mask cannot drift apart: w > 0, d > 0, <=, NaN never
                admissible, t2 = thr * thr in f32.  A model of nine zeros (the
                verification's "no model") admits nothing.
    neighbours  match_ref's rule over the admissible set only: the nearest
                train row of a query is the lowest (exact integer d^2, j)
                among its admissible j, its second neighbour the next such
                key; the nearest query of a train row is the lowest (d^2, i)
                among its admissible i; distance = sqrt((float) d^2).
    cross       query i is kept only if its nearest admissible train row's
                nearest admissible query is i.
    ratio       kept iff d1 < np.float32(r) * d2 (f32, one multiply, strict).
                A query with exactly one admissible candidate has d2 = +inf
                and PASSES.  This deliberately differs from match_ref, where
                no second neighbour means rejected: under a 3 px homography
                gate most true matches have a single candidate, and the
                unguided rule would empty the result.
    cap         max_distance > 0 keeps a query only if d1 <= max_distance
                (f32); 0 means no cap.
    no match    a query without an admissible candidate has no match.

With cross_check, no ratio test, no cap and the verification's own model and
threshold, every inlier of a verified cross-checked match set is in the guided
result: the global nearest (lowest index on ties) of a row or a column stays
the nearest of any subset that contains it.

`variant` selects a deliberately wrong restatement (test use only):
"post_filter" the gate applied to the unguided result, "lone_rejected" a sole
admissible candidate fails the ratio test, "cross_ungated" the train row's
back-neighbour taken over all queries, "gate_lt" a strict < at the threshold,
"no_w_test" no test of the homography's w > 0, "tie_high" the highest index
among equal d^2.
"""
import numpy as np

import epipolar_ref
import match_ref
import verify_ref

VARIANTS = ("post_filter", "lone_rejected", "cross_ungated", "gate_lt", "no_w_test", "tie_high")
KINDS = ("homography", "fundamental")
_BIG = 1 << 30  # above every d^2 (< 2^23); match_ref's sort key d^2 * 2^32 + index stays in int64


def _mask_fn(kind):
    if kind == "homography":
        return verify_ref.inlier_mask
    if kind == "fundamental":
        return epipolar_ref.inlier_mask
    raise ValueError(kind)


def admissible(kq, kt, g, thr, kind="homography", variant=None):
    """(nq, nt) bool: the verification's inlier test on every (query keypoint, train keypoint) record."""
    kq = np.asarray(kq, np.float32).reshape(len(kq), -1)[:, :2]
    kt = np.asarray(kt, np.float32).reshape(len(kt), -1)[:, :2]
    g = np.asarray(g, np.float32).reshape(9)
    nq, nt = len(kq), len(kt)
    rec = np.concatenate([np.repeat(kq, nt, axis=0), np.tile(kt, (nq, 1))], 1).astype(np.float32)
    fn = _mask_fn(kind)
    ok = fn(rec, g, thr, "thr_lt" if variant == "gate_lt" else None)
    if variant == "no_w_test" and kind == "homography":
        ok = ok | fn(rec, -g, thr)  # -H: the same du, dv and limit, w of the other sign
    return ok.reshape(nq, nt)


def match(dq, dt, kq, kt, g, thr, kind="homography", ratio=0.0, cross_check=True, max_distance=0.0, variant=None):
    """(query_idx, train_idx, distance) of the kept queries, in query order."""
    nq, nt = len(dq), len(dt)
    if nq == 0 or nt == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
    adm = admissible(kq, kt, g, thr, kind, variant)
    if variant == "post_filter":
        qi, ti, dist = match_ref.match(dq, dt, ratio, cross_check)
        keep = adm[qi, ti]
        if max_distance:
            keep &= dist <= np.float32(max_distance)
        return qi[keep], ti[keep], dist[keep]
    d2 = match_ref.d2_matrix(dq, dt)
    gated = np.where(adm, d2, _BIG)
    tie = "tie_high" if variant == "tie_high" else None
    idx, val = match_ref._top2(gated, tie)
    val = np.where(val >= _BIG, -1, val)  # an inadmissible "neighbour" is absent
    idx = np.where(val >= 0, idx, -1).astype(np.int32)
    dist = match_ref._dist(val)
    keep = idx[:, 0] >= 0
    if cross_check:
        back = match_ref._top2((d2 if variant == "cross_ungated" else gated).T, tie)[0][:, 0]
        keep &= back[np.maximum(idx[:, 0], 0)] == np.arange(nq)
    if ratio:
        with np.errstate(all="ignore"):
            ok = dist[:, 0] < np.float32(ratio) * dist[:, 1]  # a lone candidate: d2 = +inf, passes
        if variant == "lone_rejected":
            ok &= idx[:, 1] >= 0
        keep &= ok
    if max_distance:
        keep &= dist[:, 0] <= np.float32(max_distance)
    k = np.nonzero(keep)[0]
    return k.astype(np.int32), idx[k, 0].astype(np.int32), dist[k, 0].astype(np.float32)


# ---- fixtures ---------------------------------------------------------------
THR = 3.0


def model_h():
    """verify_ref.H_MILD as the (9,) f32 a verification returns."""
    return verify_ref.H_MILD.astype(np.float32).reshape(9)


def model_f():
    """The F of epipolar_ref's planted two-view scenes, largest entry 1, (9,) f32."""
    return epipolar_ref._scale_f32(epipolar_ref.true_f().reshape(1, 9))[0]


def _kps(xy, rng):
    k = np.zeros((len(xy), 5), np.float32)
    k[:, :2] = xy
    k[:, 2:] = rng.uniform(1, 5, (len(xy), 3))
    return k


def scene(nq, nt, seed, kind="homography"):
    """Uniform random u8 descriptors and random keypoints in 640 x 640.
    k = min(max(1, nq // 2), max(1, 3 nt // 5)) queries are planted: a train
    row at the model's place for the query (H_MILD's projection, or the second
    view of a point at depth 4..12) +-1 px, descriptor = the query's plus noise
    in [-3, 3].  The first k // 3 of them also have an exact copy of the
    query's descriptor on a train row at an inadmissible place (the unguided
    nearest is wrong), the next k // 3 a second admissible train row 1.5 px
    from the planted one with descriptor noise +-40 (a real second neighbour).
    With min(nq, nt) >= 1 at least one pair is admissible.
    -> dict: dq, dt (u8), kq, kt ((n, 5) f32), g ((9,) f32), kind, thr, and
    the planted (query, train), decoy (query, train), second (query, train)
    index arrays."""
    rng = np.random.default_rng(seed)
    g = model_h() if kind == "homography" else model_f()
    dq = rng.integers(0, 256, (nq, 128), dtype=np.uint8)
    dt = rng.integers(0, 256, (nt, 128), dtype=np.uint8)
    q_xy = rng.uniform(20, 620, (nq, 2))
    t_xy = rng.uniform(0, 640, (nt, 2))
    k = min(max(1, nq // 2), max(1, (3 * nt) // 5)) if min(nq, nt) >= 1 else 0
    n3 = k // 3
    qrows = rng.permutation(nq)[:k]
    trows = rng.permutation(nt)
    plant, decoy, second = trows[:k], trows[k:k + n3], trows[k + n3:k + 2 * n3]
    assert len(second) == n3
    if k:
        if kind == "homography":
            place = verify_ref.project(verify_ref.H_MILD, q_xy[qrows])
        else:
            place = epipolar_ref.two_view(q_xy[qrows], rng.uniform(4.0, 12.0, k))
        t_xy[plant] = place + rng.uniform(-1.0, 1.0, (k, 2))
        dt[plant] = np.clip(dq[qrows].astype(np.int64) + rng.integers(-3, 4, (k, 128)), 0, 255).astype(np.uint8)
    for i in range(n3):  # decoys: the query's own descriptor where the model forbids it
        for _ in range(1000):
            xy = rng.uniform(0, 640, (1, 2))
            if not admissible(q_xy[qrows[i]][None], xy, g, 2 * THR, kind)[0, 0]:
                break
        t_xy[decoy[i]] = xy
        dt[decoy[i]] = dq[qrows[i]]
    if n3:
        ang = rng.uniform(0, 2 * np.pi, n3)
        src = plant[n3:2 * n3]
        t_xy[second] = t_xy[src] + 1.5 * np.stack([np.cos(ang), np.sin(ang)], 1)
        dt[second] = np.clip(dq[qrows[n3:2 * n3]].astype(np.int64) + rng.integers(-40, 41, (n3, 128)),
                             0, 255).astype(np.uint8)
    return dict(dq=dq, dt=dt, kq=_kps(q_xy, rng), kt=_kps(t_xy, rng), g=g, kind=kind, thr=THR,
                planted=(qrows, plant), decoy=(qrows[:n3], decoy), second=(qrows[n3:2 * n3], second))


def sorted_by_y(s):
    """The scene with both keypoint sets (and their descriptors) in ascending y:
    admissible elements then cluster along the tiles' diagonal."""
    oq, ot = np.argsort(s["kq"][:, 1], kind="stable"), np.argsort(s["kt"][:, 1], kind="stable")
    return dict(s, dq=s["dq"][oq], kq=s["kq"][oq], dt=s["dt"][ot], kt=s["kt"][ot],
                planted=None, decoy=None, second=None)


def _background(rng, nq=6, nt=6):
    """Random rows far away from everything the variant fixtures plant (x, y >= 2000)."""
    return (rng.integers(0, 256, (nq, 128), dtype=np.uint8), rng.integers(0, 256, (nt, 128), dtype=np.uint8),
            rng.uniform(2000, 3000, (nq, 2)), rng.uniform(5000, 6000, (nt, 2)))


def _fixture(dq, dt, q_xy, t_xy, g, thr, rng, **kw):
    args = dict(ratio=0.0, cross_check=True, max_distance=0.0)
    args.update(kw)
    return dict(dq=dq, dt=dt, kq=_kps(q_xy, rng), kt=_kps(t_xy, rng), g=np.asarray(g, np.float32).reshape(9),
                kind="homography", thr=thr, args=args)


def variant_fixture(name):
    """The smallest input on which the wrong variant `name` differs from the
    rule: dict with dq, dt, kq, kt, g, kind, thr and args (ratio, cross_check,
    max_distance).  "post_filter" and "lone_rejected" use the decoy scene."""
    rng = np.random.default_rng(VARIANTS.index(name) + 100)
    if name in ("post_filter", "lone_rejected"):
        s = scene(37, 300, 5)
        return dict(s, args=dict(ratio=0.8 if name == "lone_rejected" else 0.0, cross_check=True, max_distance=0.0))
    dq, dt, q_xy, t_xy = _background(rng)
    ident = np.eye(3)
    if name == "cross_ungated":
        # train row 0 is admissible for query 0 only, but its descriptor is query 1's
        q_xy[0], t_xy[0], q_xy[1] = (100, 100), (101, 100), (400, 300)
        dq[0] = np.clip(dt[0].astype(np.int64) + rng.integers(-3, 4, 128), 0, 255).astype(np.uint8)
        dq[1] = dt[0]
        return _fixture(dq, dt, q_xy, t_xy, ident, THR, rng)
    if name == "gate_lt":
        # integer coordinates under the integer translation (+5, -3): train row 0 is exactly thr px off
        thr = 2.0
        q_xy[0], t_xy[0] = (64, 48), (64 + 5 + thr, 48 - 3)
        return _fixture(dq, dt, q_xy, t_xy, [[1, 0, 5], [0, 1, -3], [0, 0, 1]], thr, rng)
    if name == "no_w_test":
        # w = 1 - x / 128: query 0 at (384, 128) has w = -2 and "projects" to (-192, -64), behind the
        # horizon; query 1 at (64, 32) has w = 0.5 and projects to (128, 64)
        q_xy[0], t_xy[0] = (384, 128), (-192, -64)
        q_xy[1], t_xy[1] = (64, 32), (128, 64)
        return _fixture(dq, dt, q_xy, t_xy, [[1, 0, 0], [0, 1, 0], [-1 / 128, 0, 1]], THR, rng)
    if name == "tie_high":
        # two admissible train rows with one descriptor
        q_xy[0], t_xy[1], t_xy[4] = (200, 150), (201, 150), (200, 151)
        dt[4] = dt[1]
        return _fixture(dq, dt, q_xy, t_xy, ident, THR, rng, cross_check=False)
    raise ValueError(name)


def run(f, variant=None, **over):
    """match() on a scene / fixture dict; `over` replaces its args."""
    args = dict(f.get("args", {}))
    args.update(over)
    return match(f["dq"], f["dt"], f["kq"], f["kt"], f["g"], f["thr"], f["kind"], variant=variant, **args)


def verified_scene(m, share, seed):
    """A verify_ref.planted(m, share, seed) scene as a matched pair: record k
    is (query k, train perm[k]) and query k's descriptor is that train row's
    plus noise in [-3, 3], so the unguided cross-checked matches are the m
    records, a share of them inliers of H_MILD.  -> (dq, dt, kq, kt)."""
    rng = np.random.default_rng(seed + 1000)
    rec, _ = verify_ref.planted(m, share, seed)
    perm = rng.permutation(m)
    dt = rng.integers(0, 256, (m, 128), dtype=np.uint8)
    dq = np.clip(dt[perm].astype(np.int64) + rng.integers(-3, 4, (m, 128)), 0, 255).astype(np.uint8)
    t_xy = np.zeros((m, 2))
    t_xy[perm] = rec[:, 2:4]
    return dq, dt, _kps(rec[:, :2], rng), _kps(t_xy, rng)
