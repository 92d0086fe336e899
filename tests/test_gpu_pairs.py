"""Frame-pair proposal on the GPU (sift_mi_propose_pairs_device;
csrc/pairs.hip) against its numpy restatement (pairs_ref.py, pinned by
test_pairs_ref_cpu.py): the score matrix and the proposed pairs are integers
and must equal it exactly.  LABELLED EXTENSION: the crate has nothing like it.

Segment lengths and subset sizes sit around the MFMA tile (32), the wave (64)
and the workgroup tile (128), with empty and one-row subsets (no second
neighbour); the sizes take few values, so equal sizes straddle every cut."""
import ctypes
import functools

import numpy as np
import pytest

import pairs_ref as R

gpu = pytest.mark.gpu

LENS = [0, 1, 2, 31, 33, 63, 64, 65, 127, 128, 129, 300]
LENS12 = [64, 300, 0, 129, 1, 31, 128, 2, 65, 33, 127, 63]  # LENS in a mixed order
SUBSETS = [1, 2, 63, 64, 65, 127, 128]
ARENAS = {
    "n12": lambda: R.arena(LENS12, seed=12),
    "n3": lambda: R.arena([0, 65, 128], seed=3),
    "n2": lambda: R.arena([300, 1], seed=2),
    "n1": lambda: R.arena([129], seed=1),
    "hub": R.hub_arena,
    "bait128": lambda: R.bait_arena([300, 129, 64, 130], 128, seed=21)[:3],
    "bait8": lambda: R.bait_arena([40, 9, 0, 12, 30], 8, seed=21)[:3],
}


@functools.lru_cache(maxsize=None)
def _arena(name):
    """(device descriptors, device keypoints, desc, kps, offsets) of ARENAS[name]."""
    import torch
    desc, kps, offs = ARENAS[name]()
    for a in (desc, kps, offs):
        a.setflags(write=False)
    td, tk = torch.from_numpy(desc.copy()).cuda(), torch.from_numpy(kps.copy()).cuda()
    torch.cuda.synchronize()
    return td, tk, desc, kps, offs


@functools.lru_cache(maxsize=None)
def _want_scores(name, h, ratio):
    _, _, desc, kps, offs = _arena(name)
    sc = R.score_matrix(desc, kps, offs, h, ratio)
    sc.setflags(write=False)
    return sc


def _check(ctx, name, h, ratio, min_matches=8, max_partners=0):
    td, tk, desc, kps, offs = _arena(name)
    want = _want_scores(name, h, float(ratio))
    pairs, sc = ctx.propose_pairs_device(td.data_ptr(), tk.data_ptr(), offs, h, ratio, min_matches, max_partners)
    assert sc.dtype == np.uint32 and sc.shape == want.shape
    assert np.array_equal(sc, want), (name, h, ratio, np.argwhere(sc != want)[:8].tolist())
    assert pairs == R.propose(want, min_matches, max_partners), (name, h, ratio, min_matches, max_partners)
    return pairs, want


def test_lengths_cover_the_issue_set():
    assert sorted(LENS12) == LENS


@gpu
@pytest.mark.parametrize("ratio", [0.0, 0.8, 1.0])
@pytest.mark.parametrize("h", SUBSETS)
def test_all_shapes_12_segments(ctx, h, ratio):
    """Every (|S_a|, |S_b|) of min(LENS, h) in one call, both directions."""
    for mm in (1, 8):
        pairs, want = _check(ctx, "n12", h, ratio, mm)
    if ratio == 0.0:
        assert np.array_equal(want, want.T)
    if h >= 63:
        assert want.max() >= 8 and len(pairs) >= 3  # planted matches are found


@gpu
@pytest.mark.parametrize("name", ["n1", "n2", "n3"])
@pytest.mark.parametrize("h", [1, 64, 128])
def test_few_segments(ctx, name, h):
    for ratio in (0.0, 0.8):
        _check(ctx, name, h, ratio, 1)


@gpu
def test_no_second_neighbour_is_rejected(ctx):
    """Segment 1 of "n2" has one row: with a ratio no query of segment 0 is
    kept against it; without one the cross check keeps exactly one."""
    _, want = _check(ctx, "n2", 128, 0.8, 1)
    assert want[0, 1] == 0
    _, want0 = _check(ctx, "n2", 128, 0.0, 1)
    assert want0[0, 1] == 1 and want0[1, 0] == 1


@gpu
@pytest.mark.parametrize("max_partners", [0, 1, 2])
def test_partner_limit_either_not_both(ctx, max_partners):
    pairs, want = _check(ctx, "hub", 128, 0.8, 8, max_partners)
    assert pairs == [(0, 1), (0, 2), (0, 3)]
    if max_partners == 1:
        assert R.propose(want, 8, 1, variant="keep_both") == [(0, 1)]
    _check(ctx, "hub", 128, 0.8, 1, max_partners)


@gpu
@pytest.mark.parametrize("name,h", [("bait128", 128), ("bait8", 8)])
def test_bait_arena(ctx, name, h):
    """Rows ranked h + 1, rows before offsets[0] and after offsets[n_segs] are
    copies of subset rows of other segments (pairs_ref.bait_arena): a read past
    the cut or past the arena's bounds raises a score."""
    for ratio in (0.0, 0.8):
        _check(ctx, name, h, ratio, 1)
    assert _arena(name)[4][0] == 3  # the call starts inside the arena


@gpu
@pytest.mark.parametrize("name,perm", [("n12", [7, 3, 11, 0, 5, 9, 1, 10, 2, 8, 6, 4]), ("bait128", [2, 0, 3, 1])])
def test_permuted_segments_permute_scores(ctx, name, perm):
    import torch
    _, _, desc, kps, offs = _arena(name)
    d2, k2, o2 = R.permuted(desc, kps, offs, perm)
    td, tk = torch.from_numpy(d2.copy()).cuda(), torch.from_numpy(k2.copy()).cuda()
    torch.cuda.synchronize()
    for h, ratio in ((128, 0.8), (63, 0.0)):
        want = _want_scores(name, h, ratio)[np.ix_(perm, perm)]
        pairs, sc = ctx.propose_pairs_device(td.data_ptr(), tk.data_ptr(), o2, h, ratio, 8)
        assert np.array_equal(sc, want)
        assert pairs == R.propose(want, 8)


@gpu
def test_pair_counters_grow_by_tiles(ctx):
    ctx.reset_stats()
    assert ctx.pair_counters() == {"kernel_ms": 0.0, "tiles": 0}
    td, tk, _, _, offs = _arena("n12")
    ctx.propose_pairs_device(td.data_ptr(), tk.data_ptr(), offs)
    c1 = ctx.pair_counters()
    assert c1["tiles"] == 66 and c1["kernel_ms"] > 0
    td, tk, _, _, offs = _arena("n3")
    ctx.propose_pairs_device(td.data_ptr(), tk.data_ptr(), offs)
    td, tk, _, _, offs = _arena("n1")
    ctx.propose_pairs_device(td.data_ptr(), tk.data_ptr(), offs)
    c2 = ctx.pair_counters()
    assert c2["tiles"] == 69 and c2["kernel_ms"] > c1["kernel_ms"]
    ctx.reset_stats()
    assert ctx.pair_counters()["tiles"] == 0


@gpu
def test_argument_errors(pkg, ctx):
    from sift_features_amd import _lib
    td, tk, desc, kps, offs = _arena("n3")
    d, k = td.data_ptr(), tk.data_ptr()
    bad = {
        "subset 0": dict(subset=0), "subset 129": dict(subset=129), "ratio > 1": dict(ratio=1.5),
        "ratio < 0": dict(ratio=-0.1), "ratio nan": dict(ratio=float("nan")), "min_matches 0": dict(min_matches=0),
    }
    for what, kw in bad.items():
        with pytest.raises(pkg.SiftMiError) as e:
            ctx.propose_pairs_device(d, k, offs, **kw)
        assert e.value.code == -1, what
    for what, args in {"offsets decrease": (d, k, [0, 65, 3, 193]), "d_desc misaligned": (d + 8, k, offs),
                       "d_kps misaligned": (d, k + 2, offs), "n_segs > 4096": (d, k, [0] * 4098)}.items():
        with pytest.raises(pkg.SiftMiError) as e:
            ctx.propose_pairs_device(*args)
        assert e.value.code == -1, what
    # n_segs of 0 or 1: no pairs
    assert ctx.propose_pairs_device(d, k, [5])[0] == []
    pairs, sc = ctx.propose_pairs_device(d, k, [0, 65])
    assert pairs == [] and sc.tolist() == [[0]]
    # cap too small: EINVAL with *n_pairs set, scores written
    want = R.propose(_want_scores("n12", 128, 0.0), 1)
    td, tk, _, _, offs = _arena("n12")
    c_offs = (ctypes.c_size_t * len(offs))(*[int(v) for v in offs])
    prm = _lib.PairParams(128, 0.0, 1, 0)
    out = (_lib.SegPair * len(want))()
    n = ctypes.c_size_t(0)
    sc = np.zeros((12, 12), np.uint32)
    L = pkg.lib()
    rc = L.sift_mi_propose_pairs_device(ctx._h, td.data_ptr(), tk.data_ptr(), c_offs, 12, ctypes.byref(prm),
                                        sc.ctypes.data, out, len(want) - 1, ctypes.byref(n))
    assert rc == -1 and n.value == len(want) > 1 and np.array_equal(sc, _want_scores("n12", 128, 0.0))
    assert out[len(want) - 1].train_seg == 0  # nothing written past cap
    rc = L.sift_mi_propose_pairs_device(ctx._h, td.data_ptr(), tk.data_ptr(), c_offs, 12, ctypes.byref(prm), None, out,
                                        len(want), ctypes.byref(n))
    assert rc == 0 and [(out[i].query_seg, out[i].train_seg) for i in range(n.value)] == want


# ---- the chain's entry: frames of two scenes, unordered ---------------------------
@gpu
def test_scene_proposal_from_batch_results(pkg, synth):
    """Ten 320 x 240 crops, five of each of two 640 x 240 scenes at x = 0, 60,
    .., 240 (neighbours overlap by 81 %, the outermost two by 25 %).  First the
    fixture on the restatement alone (same-scene scores >= 8 > cross-scene),
    then the GPU against the restatement, then the proposal."""
    import torch
    from test_gpu_configs import _device_results
    frames = np.stack([synth.frame(640, 240, seed)[:, x:x + 320] for seed in (1, 2) for x in range(0, 241, 60)])
    t = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    torch.cuda.synchronize()
    c2 = pkg.Context(0, pkg.OpenCVProcessing)
    try:
        offs, _ = c2.sift_batch_device(t.data_ptr(), 10, 320, 240, t.stride(1), t.stride(0), fetch=False)
        before = c2.device_results()
        pairs, sc = c2.propose_frames(offs, subset=128, ratio=0.8, min_matches=8)
        assert c2.device_results() == before  # only read
        kps, desc = _device_results(c2, int(offs[-1]))
    finally:
        c2.close()
    want_pairs, want = R.run(desc, kps, offs, 128, 0.8, 8)
    same = np.zeros((10, 10), bool)
    same[:5, :5] = same[5:, 5:] = True
    off_diag = ~np.eye(10, dtype=bool)
    s = np.maximum(want, want.T)
    print("same-scene scores", s[same & off_diag].min(), "..", s[same & off_diag].max(),
          "cross-scene", s[~same].min(), "..", s[~same].max())
    assert (s[same & off_diag] >= 8).all() and (s[~same] < 8).all()
    assert np.array_equal(sc, want)
    assert pairs == want_pairs == [(a, b) for a in range(10) for b in range(a + 1, 10) if same[a, b]]
    assert len(pairs) == 20
