"""Guided matching on the GPU (sift_mi_match_pairs_guided_device,
sift_mi_match_guided; csrc/match_guided.hip) against its numpy restatement
guided_ref.py.  Everything is bit-exact -- indices and pair offsets equal, f32
distances equal as bit patterns -- and every case runs with the wave-level
cull on and off."""
import ctypes
import functools

import numpy as np
import pytest

import guided_ref as G
import match_ref

gpu = pytest.mark.gpu

SHAPES = [(1, 1), (5, 1), (1, 2), (37, 300), (128, 128), (129, 257), (300, 129)]
# ratio x cross check, and one case with a distance cap
SETTINGS = [dict(ratio=0.0, cross_check=True), dict(ratio=0.0, cross_check=False), dict(ratio=0.8, cross_check=True),
            dict(ratio=0.8, cross_check=False), dict(ratio=0.8, cross_check=True, max_distance=300.0)]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and \
        np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


@functools.lru_cache(maxsize=None)
def _scene(nq, nt, kind):
    s = G.scene(nq, nt, nq * 7 + nt, kind)
    for k in ("dq", "dt", "kq", "kt", "g"):
        s[k].setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _ref(nq, nt, kind, setting):
    return G.run(_scene(nq, nt, kind), **SETTINGS[setting])


def _gpu(ctx, f, **args):
    """The one-pair host-array call on a scene / fixture dict, cull on and off: both must agree."""
    a = dict(f.get("args", {}))
    a.update(args)
    out = []
    for cull in (1, 0):
        with ctx.path_options(guided_cull=cull):
            out.append(ctx.match_guided(f["dq"], f["kq"], f["dt"], f["kt"], f["g"], threshold=f["thr"],
                                        model=f["kind"], **a))
    assert _same(out[0], out[1]), "cull on != cull off"
    return out[0]


# ---- shape grid ---------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("nq,nt", SHAPES)
def test_shape_grid(ctx, nq, nt, kind):
    s = _scene(nq, nt, kind)
    assert G.admissible(s["kq"], s["kt"], s["g"], s["thr"], kind).any()
    for i, setting in enumerate(SETTINGS):
        want = _ref(nq, nt, kind, i)
        got = _gpu(ctx, s, **setting)
        assert got[0].dtype == np.int32 and got[2].dtype == np.float32
        assert _same(got, want), (setting, len(got[0]), len(want[0]))
    assert len(_ref(nq, nt, kind, 1)[0]) > 0  # every shape has a match without the cross check


@gpu
@pytest.mark.parametrize("name", G.VARIANTS)
def test_variant_fixtures(ctx, name):
    """The GPU gives the rule's result where each wrong variant differs from it."""
    f = G.variant_fixture(name)
    want = G.run(f)
    assert not _same(want, G.run(f, variant=name))
    assert _same(_gpu(ctx, f), want), name


@gpu
def test_zero_model_and_empty_sides(ctx):
    s = _scene(37, 300, "homography")
    zero = dict(s, g=np.zeros(9, np.float32))
    assert len(_gpu(ctx, zero, cross_check=False)[0]) == 0
    e, ek = np.zeros((0, 128), np.uint8), np.zeros((0, 5), np.float32)
    assert len(_gpu(ctx, dict(s, dq=e, kq=ek))[0]) == 0
    assert len(_gpu(ctx, dict(s, dt=e, kt=ek))[0]) == 0


# ---- segment arena --------------------------------------------------------------------
SEG_LENS, PAIRS = match_ref.SEG_LENS, match_ref.PAIRS
ZERO_PAIR = 6  # (3, 3), in the middle of PAIRS: an all-zero model
PLACES = np.array([[40 + 70 * k, 50 + 45 * k] for k in range(8)], np.float32)


def _arena_kps(offs):
    """Row i of every segment sits at PLACES[i % 8]: under the identity a query
    competes for every eighth train row, and the rows just past a segment --
    its neighbour's copies of its own edge rows (match_ref.segment_arena: up to
    8 of them) -- sit at admissible places with in-segment descriptors."""
    kps = np.zeros((int(offs[-1]), 5), np.float32)
    for s in range(len(offs) - 1):
        n = int(offs[s + 1] - offs[s])
        kps[offs[s]:offs[s + 1], :2] = PLACES[np.arange(n) % 8]
    kps[:, 2:] = 1.0
    return kps


@pytest.fixture(scope="module")
def arena_dev():
    import torch
    rows, offs = match_ref.segment_arena()
    kps = _arena_kps(offs)
    d, k = torch.from_numpy(rows.copy()).cuda(), torch.from_numpy(kps.copy()).cuda()
    torch.cuda.synchronize()
    return d, k, rows, kps, offs


def _arena_models(kind):
    g = np.eye(3, dtype=np.float32).reshape(9) if kind == "homography" else G.model_f()
    models = [g.reshape(3, 3).copy() for _ in PAIRS]
    models[ZERO_PAIR] = np.zeros((3, 3), np.float32)
    return models


@gpu
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("setting", range(len(SETTINGS)))
def test_segment_arena(ctx, arena_dev, setting, kind):
    d, k, rows, kps, offs = arena_dev
    models = _arena_models(kind)
    got = []
    for cull in (1, 0):
        with ctx.path_options(guided_cull=cull):
            got.append(ctx.match_pairs_guided_device(d.data_ptr(), k.data_ptr(), offs, PAIRS, models, threshold=G.THR,
                                                     model=kind, **SETTINGS[setting]))
    assert len(got[0]) == len(PAIRS)
    total = 0
    for p, (a, b) in enumerate(PAIRS):
        q, tr = slice(offs[a], offs[a + 1]), slice(offs[b], offs[b + 1])
        want = G.match(rows[q], rows[tr], kps[q], kps[tr], models[p], G.THR, kind, **SETTINGS[setting])
        assert _same(got[0][p], want), (a, b, len(got[0][p][0]), len(want[0]))
        assert _same(got[1][p], want), ("cull off", a, b)
        total += len(want[0])
    assert len(got[0][ZERO_PAIR][0]) == 0  # no model: an empty range
    assert _same(got[0][PAIRS.index((5, 2))], got[0][-1])  # the pair listed twice
    assert total > 0


def _raw(pkg, ctx, d_desc, d_kps, offs, pairs, kind, models, prm, cap):
    from sift_features_amd import _lib
    L = pkg.lib()
    c_offs = None if offs is None else (ctypes.c_size_t * len(offs))(*[int(v) for v in offs])
    c_pairs = None if pairs is None else (_lib.SegPair * max(1, len(pairs)))(*[_lib.SegPair(a, b) for a, b in pairs])
    n_pairs = 0 if pairs is None else len(pairs)
    c_models = None if models is None else np.ascontiguousarray(models, np.float32).ctypes.data
    c_prm = None if prm is None else ctypes.byref(_lib.GuidedParams(*prm))
    out = (_lib.Match * max(cap, 1))()
    po = (ctypes.c_size_t * (n_pairs + 1))(*([12345] * (n_pairs + 1)))
    rc = L.sift_mi_match_pairs_guided_device(ctx._h, ctypes.c_void_p(d_desc), ctypes.c_void_p(d_kps), c_offs,
                                             0 if offs is None else len(offs) - 1, c_pairs, n_pairs, kind, c_models,
                                             c_prm, out, cap, po)
    return rc, out, list(po)


@gpu
def test_pair_offsets_and_cap(pkg, ctx, arena_dev):
    d, k, rows, kps, offs = arena_dev
    models = _arena_models("homography")
    want = [G.match(rows[offs[a]:offs[a + 1]], rows[offs[b]:offs[b + 1]], kps[offs[a]:offs[a + 1]],
                    kps[offs[b]:offs[b + 1]], models[p], G.THR) for p, (a, b) in enumerate(PAIRS)]
    counts = [len(w[0]) for w in want]
    total = sum(counts)
    assert total > 0
    prm = (G.THR, 0.0, 0.0, 1)
    rc, out, po = _raw(pkg, ctx, d.data_ptr(), k.data_ptr(), offs, PAIRS, 0, models, prm, total)
    assert rc == 0 and po == [0] + list(np.cumsum(counts))
    a = np.ctypeslib.as_array(out)[:total]
    assert np.array_equal(a["query_idx"], np.concatenate([w[0] for w in want]))
    assert np.array_equal(a["train_idx"], np.concatenate([w[1] for w in want]))
    # cap too small: EINVAL, the needed count in pair_offsets[n_pairs]
    rc, _, po = _raw(pkg, ctx, d.data_ptr(), k.data_ptr(), offs, PAIRS, 0, models, prm, total - 1)
    assert rc == -1 and po[-1] == total
    assert b"cap" in pkg.lib().sift_mi_last_error()
    rc, _, po = _raw(pkg, ctx, d.data_ptr(), k.data_ptr(), offs, [], 0, np.zeros(9), prm, 0)
    assert rc == 0 and po == [0]


@gpu
def test_guided_einval(pkg, ctx, arena_dev):
    d, k, rows, kps, offs = arena_dev
    dp, kp, n_seg, ok_pairs, cap = d.data_ptr(), k.data_ptr(), len(offs) - 1, [(1, 2)], 1000
    eye = np.eye(3, dtype=np.float32).reshape(1, 9)
    ok = (3.0, 0.8, 0.0, 1)
    call = lambda **kw: _raw(pkg, ctx, **{**dict(d_desc=dp, d_kps=kp, offs=offs, pairs=ok_pairs, kind=0, models=eye,
                                                 prm=ok, cap=cap), **kw})[0]
    assert call() == 0
    # null arguments
    for name in ("d_desc", "d_kps", "offs", "pairs", "models", "prm"):
        assert call(**{name: None}) == -1, name
    # an unknown kind
    assert call(kind=2) == -1 and call(kind=-1) == -1
    # threshold: not finite, or <= 0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(prm=(bad, 0.8, 0.0, 1)) == -1, bad
    # ratio, as sift_mi_match_ratio
    for bad in (float("nan"), -0.5, 1.0001, float("inf")):
        assert call(prm=(3.0, bad, 0.0, 1)) == -1, bad
    # max_distance: negative or NaN
    for bad in (-1.0, float("nan")):
        assert call(prm=(3.0, 0.8, bad, 1)) == -1, bad
    # a model entry that is not finite
    for bad in (float("nan"), float("inf")):
        m = eye.copy()
        m[0, 4] = bad
        assert call(models=m) == -1, bad
    # a pair index >= n_segs, decreasing offsets
    assert call(pairs=[(1, n_seg)]) == -1 and call(pairs=[(n_seg, 1)]) == -1
    assert call(offs=[0, 10, 5, 20], pairs=[(0, 1)]) == -1
    with pytest.raises(ValueError):
        ctx.match_guided(rows[:3], kps[:3], rows[:3], kps[:3], eye, model="affine")
    # still usable afterwards
    assert call() == 0


# ---- the cull ---------------------------------------------------------------------------
@gpu
def test_cull_counters(ctx):
    s = G.sorted_by_y(_scene(300, 129, "homography"))
    want = G.run(s, ratio=0.8, cross_check=True)
    assert len(want[0]) > 20
    ctx.reset_stats()
    assert ctx.guided_counters() == {"tiles": 0, "culled_waves": 0}
    with ctx.path_options(guided_cull=1):
        on = ctx.match_guided(s["dq"], s["kq"], s["dt"], s["kt"], s["g"], threshold=s["thr"], ratio=0.8)
    c = ctx.guided_counters()
    print("cull on:", c)
    assert c["tiles"] == 6 and 0 < c["culled_waves"] < 4 * c["tiles"]
    ctx.reset_stats()
    with ctx.path_options(guided_cull=0):
        off = ctx.match_guided(s["dq"], s["kq"], s["dt"], s["kt"], s["g"], threshold=s["thr"], ratio=0.8)
    assert ctx.guided_counters() == {"tiles": 6, "culled_waves": 0}
    assert _same(on, want) and _same(off, want)
    # the kernels' time lands in match_ms
    assert ctx.stats()["match_ms"] > 0
    ctx.reset_stats()
    assert ctx.guided_counters() == {"tiles": 0, "culled_waves": 0}


# ---- end to end ---------------------------------------------------------------------------
@gpu
def test_match_frames_guided_end_to_end(pkg, ctx, synth):
    """Extraction, matching, verification and the guided re-match without the
    keypoints or descriptors leaving HBM; the restatement runs on the fetched
    arrays."""
    import torch
    img = synth.frame(320, 213, 7)
    frames = np.stack([img, np.roll(img, 7, axis=1), np.roll(img, (5, -9), axis=(0, 1))])
    host = ctx.sift_batch(frames)
    t = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    c2 = pkg.Context(0, pkg.OpenCVProcessing)
    try:
        offs, _ = c2.sift_batch_device(t.data_ptr(), 3, 320, 213, t.stride(1), t.stride(0), fetch=False)
        assert [int(offs[i + 1] - offs[i]) for i in range(3)] == [len(r) for r in host]
        before = c2.device_results()
        pairs = [(0, 1), (1, 2), (0, 2)]
        matches = c2.match_frames(offs, pairs, ratio=0.8)
        verified = c2.verify_frames(offs, pairs, matches)
        model = "homography"
        for kw in (dict(), dict(ratio=0.8, max_distance=250.0)):
            guided = c2.match_frames_guided(offs, pairs, verified, threshold=3.0, model=model, **kw)
            assert c2.device_results() == before  # only read
            for (a, b), mt, (H, mask, info), g in zip(pairs, matches, verified, guided):
                assert info["best_hypothesis"] >= 0 and info["n_inliers"] >= 8
                kq, kt = host[a].keypoints_array, host[b].keypoints_array
                want = G.match(host[a].descriptors, host[b].descriptors, kq, kt, H, 3.0, model, cross_check=True,
                               **kw)
                print(f"pair {(a, b)} {kw}: {len(mt[0])} matches, {info['n_inliers']} inliers, {len(g[0])} guided")
                assert _same(g, want), (a, b, len(g[0]), len(want[0]))
                assert G.admissible(kq, kt, H, 3.0, model)[g[0], g[1]].all()
                if not kw:  # cross check only: every verified inlier is there
                    have = set(zip(g[0].tolist(), g[1].tolist()))
                    assert set(zip(mt[0][mask].tolist(), mt[1][mask].tolist())) <= have
                    assert len(have) >= info["n_inliers"]
    finally:
        c2.close()


@gpu
def test_sift_match_cli_guided(pkg, ctx):
    """sift_match.py --verify --guided: the four lines of test_sift_match_cli_verify, then a fifth
    with Context.match_guided's count."""
    import os
    import subprocess
    import sys
    from conftest import GOLDEN, ROOT
    paths = [os.path.join(GOLDEN, "jpeg", n + ".jpg") for n in ("bird_small", "tree_small")]
    cmd = [sys.executable, os.path.join(ROOT, "sift-features_amd", "sift_match.py"), *paths, "--processing", "opencv",
           "--ratio", "0.8", "--verify", "3"]
    out = subprocess.run(cmd + ["--guided"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    res = []
    for path in paths:
        with open(path, "rb") as f:
            res.append(ctx.sift_jpeg(f.read()))
    m = ctx.match_descriptors(res[1].descriptors, res[0].descriptors, cross_check=True, ratio=0.8)
    H, _, info = ctx.verify_matches(res[1].keypoints_array, res[0].keypoints_array, m, threshold=3.0)
    g = ctx.match_guided(res[1].descriptors, res[1].keypoints_array, res[0].descriptors, res[0].keypoints_array, H,
                         threshold=3.0)
    assert _same(g, G.match(res[1].descriptors, res[0].descriptors, res[1].keypoints_array, res[0].keypoints_array,
                            H, 3.0))
    lines = out.stdout.split("\n")
    assert lines[:5] == ["225 keypoints", "1270 keypoints", f"{len(m[0])} matches (ratio 0.8)",
                         f"{info['n_inliers']} inliers (homography, threshold 3)", f"{len(g[0])} guided matches"]
    assert lines[5:] == [""]
