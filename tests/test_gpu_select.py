"""Spread-limited selection on the GPU (sift_mi_select_spread_device;
csrc/select.hip) against its numpy restatement (select_ref.py, pinned by
test_select_ref_cpu.py): sel_offsets, rows, every radius (as its bit pattern)
and the compact arena must equal it exactly.  LABELLED EXTENSION: the crate
has nothing like it.

Segment lengths sit around the wave (64), the workgroup (256), the radius
kernel's candidates per LDS stage (C) and its query rows per workgroup (512),
with empty, one-row and two-row segments; the limits around the same sizes
and around the longest segment; the grid arenas take few responses and
positions, so equal radii and equal responses straddle every cut."""
import ctypes
import functools

import numpy as np
import pytest

import match_ref
import pairs_ref
import select_ref as R

gpu = pytest.mark.gpu

C = 1024  # csrc/select_rule.h kSelectChunk: candidates per LDS stage of k_select_radius
LENS = [0, 1, 2, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 1]
MIXED = [64, 2 * C + 1, 0, 257, 1, C, 63, 256, 2, C + 1, 65, C - 1, 255]  # LENS in a mixed order
PERM = [7, 3, 11, 0, 5, 9, 1, 12, 10, 2, 8, 6, 4]
N_MAX = max(LENS)
LIMITS = [1, 2, 64, 255, 256, 257, N_MAX - 1, N_MAX, N_MAX + 1, 2 ** 31 - 1]
CS = [0.9, 1.0, 0.5]
ARENAS = {
    "grid": lambda: R.arena(MIXED, 11, "grid"),
    "float": lambda: R.arena(MIXED, 12, "float"),
    "bait": lambda: R.bait_arena(MIXED, 13, "float", base=3, tail=3),
    "bait_grid": lambda: R.bait_arena(MIXED, 14, "grid", base=3, tail=3),
    "fused": R.fused_fixture,
}


def _read(ptr, shape, dtype):
    out = np.empty(shape, dtype)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    if out.nbytes:
        assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


@functools.lru_cache(maxsize=None)
def _arena(name):
    """(device keypoints, device descriptors, kps, desc, offsets) of ARENAS[name]; the buffers hold every row."""
    import torch
    kps, offs = ARENAS[name]()
    desc = np.random.default_rng(len(kps)).integers(0, 256, (len(kps), 128), dtype=np.uint8)
    for a in (kps, desc, offs):
        a.setflags(write=False)
    tk, td = torch.from_numpy(kps.copy()).cuda(), torch.from_numpy(desc.copy()).cuda()
    torch.cuda.synchronize()
    return tk, td, kps, desc, offs


@functools.lru_cache(maxsize=None)
def _want_r2(name, c):
    _, _, kps, _, offs = _arena(name)
    r2 = R.radius2(kps, offs, c)
    r2.setflags(write=False)
    return r2


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(ctx, name, limit, c, desc=True, radius2=True):
    tk, td, kps, dsc, offs = _arena(name)
    want_r2 = _want_r2(name, float(c))
    want_sel, want_rows = R.pick(want_r2, offs, limit)
    sel = ctx.select_spread_device(tk.data_ptr(), td.data_ptr() if desc else None, offs, limit, c, radius2=radius2)
    assert np.array_equal(sel.offsets, want_sel), (name, limit, c)
    assert sel.rows.dtype == np.uint32 and np.array_equal(sel.rows, want_rows), (name, limit, c)
    if radius2:
        bad = np.nonzero(_bits(sel.radius2) != _bits(want_r2))[0]
        assert len(sel.radius2) == len(want_r2) and not len(bad), (name, limit, c, bad[:8].tolist())
    else:
        assert sel.radius2 is None
    src = R.arena_rows(offs, want_sel, want_rows)
    assert np.array_equal(_read(sel.d_kps_ptr, (len(src), 5), np.float32).view(np.uint32), kps[src].view(np.uint32))
    if desc:
        assert np.array_equal(_read(sel.d_desc_ptr, (len(src), 128), np.uint8), dsc[src])
    else:
        assert sel.d_desc_ptr is None
    return sel


def test_lengths_and_limits_cover_the_issue_set():
    assert sorted(MIXED) == LENS and sorted(PERM) == list(range(len(LENS)))
    assert {1, 2, 64, 255, 256, 257, 2 ** 31 - 1} <= set(LIMITS) and max(LENS) < 5000


@gpu
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("name", ["grid", "float"])
def test_all_lengths_one_arena(ctx, name, limit, c):
    sel = _check(ctx, name, limit, c)
    if name == "grid" and limit == 64 and c == 0.9:  # equal radii straddle the cut of the longest segment
        s = MIXED.index(N_MAX)
        _, _, _, _, offs = _arena(name)
        r2 = sel.radius2[offs[s]:offs[s + 1]]
        cut = r2[sel.segment_rows(s)].min()
        assert (r2 == cut).sum() > (r2[sel.segment_rows(s)] == cut).sum() > 0


@gpu
@pytest.mark.parametrize("name", ["grid", "float"])
def test_permuted_segments(ctx, name):
    import torch
    _, _, kps, _, offs = _arena(name)
    k2, o2 = R.permuted(kps, offs, PERM)
    tk = torch.from_numpy(k2.copy()).cuda()
    torch.cuda.synchronize()
    for limit, c in ((64, 0.9), (257, 1.0)):
        want_r2 = _want_r2(name, c)
        want_sel, want_rows = R.pick(want_r2, offs, limit)
        sel = ctx.select_spread_device(tk.data_ptr(), None, o2, limit, c)
        for i, p in enumerate(PERM):
            assert np.array_equal(sel.segment_rows(i), want_rows[want_sel[p]:want_sel[p + 1]]), (i, p)
            assert np.array_equal(_bits(sel.radius2[o2[i]:o2[i + 1]]), _bits(want_r2[offs[p]:offs[p + 1]])), (i, p)


@gpu
@pytest.mark.parametrize("name", ["bait", "bait_grid"])
def test_bait_arena(ctx, name):
    """Rows just past every segment bound and outside the arena's first and
    last row (the buffer holds three more on either side) sit on the
    neighbouring segment's keypoints with huge responses: a read past a bound
    lowers a radius to 0 and changes `rows` (select_ref.bait_arena)."""
    for limit, c in ((8, 0.9), (64, 1.0), (257, 0.5)):
        _check(ctx, name, limit, c)
    offs = _arena(name)[4]
    assert offs[0] == 3 and len(_arena(name)[2]) == offs[-1] + 3  # the call starts and ends inside the buffer


@gpu
def test_no_descriptors_and_no_radius(ctx):
    for name in ("grid", "float"):
        a = _check(ctx, name, 64, 0.9)
        rows = a.rows.copy()
        b = _check(ctx, name, 64, 0.9, desc=False)
        c = _check(ctx, name, 64, 0.9, radius2=False)
        d = _check(ctx, name, 64, 0.9, desc=False, radius2=False)
        for other in (b, c, d):
            assert np.array_equal(other.rows, rows) and np.array_equal(other.offsets, a.offsets)


@gpu
def test_fused_fixture(ctx):
    """Separately rounded products: rows 1 and 2 tie at 1e6 and row 1 is kept;
    an fma would move row 1's or row 2's radius by one unit in the last place
    and keep row 2."""
    sel = _check(ctx, "fused", 2, 0.9)
    assert sel.rows.tolist() == [0, 1] and sel.radius2.tolist() == [np.inf, 1e6, 1e6]


@gpu
def test_host_form_and_counters(ctx):
    _, _, kps, _, offs = _arena("float")
    s = MIXED.index(N_MAX)
    k = kps[offs[s]:offs[s + 1]]
    ctx.reset_stats()
    assert ctx.select_counters() == {"kernel_ms": 0.0, "pair_tests": 0}
    for limit, c in ((100, 0.9), (N_MAX + 5, 1.0)):
        rows, r2 = ctx.select_keypoints(k, limit, c)
        want_sel, want_rows, want_r2 = R.run(k, [0, len(k)], limit, c)
        assert np.array_equal(rows, want_rows) and np.array_equal(_bits(r2), _bits(want_r2))
    c1 = ctx.select_counters()
    assert c1["pair_tests"] == 2 * N_MAX * N_MAX and c1["kernel_ms"] > 0
    rows, r2 = ctx.select_keypoints(np.zeros((0, 5), np.float32), 10)
    assert len(rows) == 0 and len(r2) == 0
    _check(ctx, "float", 64, 0.9)
    assert ctx.select_counters()["pair_tests"] == c1["pair_tests"] + sum(n * n for n in LENS)
    ctx.reset_stats()
    assert ctx.select_counters()["pair_tests"] == 0


@gpu
def test_hand_over_to_the_matcher(ctx):
    """match_pairs_device on the compact arena, mapped back through `rows`,
    equals match_ref on the gathered numpy rows."""
    import torch
    desc, kps, offs = pairs_ref.arena([300, 129, 0, 200, 64], seed=7)
    tk, td = torch.from_numpy(kps.copy()).cuda(), torch.from_numpy(desc.copy()).cuda()
    torch.cuda.synchronize()
    sel = ctx.select_spread_device(tk.data_ptr(), td.data_ptr(), offs, 100, 0.9)
    want_sel, want_rows, _ = R.run(kps, offs, 100, 0.9)
    assert np.array_equal(sel.offsets, want_sel) and np.array_equal(sel.rows, want_rows)
    pairs = [(0, 1), (1, 3), (3, 4), (4, 0), (2, 1)]
    got = ctx.match_pairs_device(sel.d_desc_ptr, sel.offsets, pairs, ratio=0.8, cross_check=True)
    src = R.arena_rows(offs, want_sel, want_rows)
    kept = 0
    for (a, b), (qi, ti, dist) in zip(pairs, got):
        ra, rb = src[want_sel[a]:want_sel[a + 1]], src[want_sel[b]:want_sel[b + 1]]
        wq, wt, wd = match_ref.match(desc[ra], desc[rb], 0.8, cross_check=True)
        # back to the original keypoints of the two segments
        assert np.array_equal(sel.segment_rows(a)[qi], (ra - offs[a])[wq]), (a, b)
        assert np.array_equal(sel.segment_rows(b)[ti], (rb - offs[b])[wt]), (a, b)
        assert np.array_equal(dist, wd)
        kept += len(qi)
    assert kept > 10  # planted matches survive the selection


@gpu
def test_argument_errors_and_small_cap(pkg, ctx):
    from sift_features_amd import _lib
    tk, td, kps, _, offs = _arena("float")
    k, d = tk.data_ptr(), td.data_ptr()
    for what, kw in {"limit 0": dict(limit=0), "c 0": dict(limit=5, c=0.0), "c > 1": dict(limit=5, c=1.01),
                     "c nan": dict(limit=5, c=float("nan")), "c < 0": dict(limit=5, c=-0.5)}.items():
        with pytest.raises(pkg.SiftMiError) as e:
            ctx.select_spread_device(k, d, offs, **kw)
        assert e.value.code == -1, what
    for what, args in {"offsets decrease": (k, d, [0, 65, 3, 193]), "d_kps misaligned": (k + 2, d, offs),
                       "d_desc misaligned": (k, d + 8, offs)}.items():
        with pytest.raises(pkg.SiftMiError) as e:
            ctx.select_spread_device(*args, 5)
        assert e.value.code == -1, what
    # no segments, and only empty ones
    sel = ctx.select_spread_device(k, d, [5], 10)
    assert sel.offsets.tolist() == [0] and len(sel.rows) == 0
    sel = ctx.select_spread_device(k, d, [5, 5, 5], 10)
    assert sel.offsets.tolist() == [0, 0, 0] and len(sel.rows) == 0 and len(sel.radius2) == 0
    # cap too small: EINVAL with the count needed in sel_offsets[n_segs], rows untouched
    want_sel, want_rows = R.pick(_want_r2("float", 0.9), offs, 64)
    L = pkg.lib()
    n = len(offs) - 1
    c_offs = (ctypes.c_size_t * (n + 1))(*[int(v) for v in offs])
    c_sel = (ctypes.c_size_t * (n + 1))()
    rows = np.full(len(want_rows), 0xFFFFFFFF, np.uint32)
    prm = _lib.SelectParams(64, 0.9)
    rc = L.sift_mi_select_spread_device(ctx._h, k, d, c_offs, n, ctypes.byref(prm), c_sel, rows.ctypes.data,
                                        len(want_rows) - 1, None)
    assert rc == -1 and c_sel[n] == len(want_rows) > 1 and list(c_sel) == want_sel.tolist()
    assert (rows == 0xFFFFFFFF).all()
    rc = L.sift_mi_select_spread_device(ctx._h, k, d, c_offs, n, ctypes.byref(prm), c_sel, rows.ctypes.data,
                                        len(want_rows), None)
    assert rc == 0 and np.array_equal(rows, want_rows)
    nr = ctypes.c_size_t()
    seg = np.ascontiguousarray(kps[offs[1]:offs[2]])
    rc = L.sift_mi_select_keypoints(ctx._h, seg.ctypes.data, len(seg), ctypes.byref(prm), rows.ctypes.data, 63,
                                    ctypes.byref(nr), None)
    assert rc == -1 and nr.value == 64


@gpu
def test_select_frames_from_batch_results(pkg, synth):
    """Two 320 x 240 crops of one scene, extracted with the results left on
    the device, then select_frames: the restatement on the fetched keypoints,
    the extraction's results untouched, and the compact arena matched."""
    import torch
    from test_gpu_configs import _device_results
    scene = synth.frame(400, 240, 3)
    frames = np.stack([scene[:, :320], scene[:, 40:360]])
    t = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    torch.cuda.synchronize()
    c2 = pkg.Context(0, pkg.OpenCVProcessing)
    try:
        offs, _ = c2.sift_batch_device(t.data_ptr(), 2, 320, 240, t.stride(1), t.stride(0), fetch=False)
        before = c2.device_results()
        sel = c2.select_frames(offs, 100, 0.9)
        assert c2.device_results() == before  # only read
        kps, desc = _device_results(c2, int(offs[-1]))
        got_kps = _read(sel.d_kps_ptr, (len(sel), 5), np.float32)
        got_desc = _read(sel.d_desc_ptr, (len(sel), 128), np.uint8)
        (qi, ti, dist), = c2.match_pairs_device(sel.d_desc_ptr, sel.offsets, [(0, 1)], ratio=0.8)
    finally:
        c2.close()
    assert min(np.diff(offs)) > 100
    want_sel, want_rows, want_r2 = R.run(kps, offs, 100, 0.9)
    assert np.array_equal(sel.offsets, want_sel) and np.array_equal(sel.rows, want_rows)
    assert np.array_equal(_bits(sel.radius2), _bits(want_r2))
    src = R.arena_rows(offs, want_sel, want_rows)
    assert np.array_equal(got_kps.view(np.uint32), kps[src].view(np.uint32)) and np.array_equal(got_desc, desc[src])
    wq, wt, wd = match_ref.match(desc[src[:100]], desc[src[100:]], 0.8, cross_check=True)
    assert np.array_equal(qi, wq) and np.array_equal(ti, wt) and np.array_equal(dist, wd)


@gpu
def test_sift_match_cli_spread(pkg, ctx):
    """sift_match.py --spread N: both images cut to N spread keypoints before
    matching; the counts are those of the restatement's rows."""
    import os
    import subprocess
    import sys
    from conftest import GOLDEN, ROOT
    paths = [os.path.join(GOLDEN, "jpeg", n + ".jpg") for n in ("bird_small", "tree_small")]
    cmd = [sys.executable, os.path.join(ROOT, "sift-features_amd", "sift_match.py"), *paths, "--processing", "opencv",
           "--ratio", "0.8", "--spread", "150"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    res = []
    for path in paths:
        with open(path, "rb") as f:
            res.append(ctx.sift_jpeg(f.read()))
    rows = [R.run(r.keypoints_array, [0, len(r)], 150, 0.9)[1] for r in res]
    wq, _, _ = match_ref.match(res[1].descriptors[rows[1]], res[0].descriptors[rows[0]], 0.8, cross_check=True)
    assert out.stdout.split("\n") == ["225 keypoints", "1270 keypoints", "150 and 150 kept (spread 150)",
                                      f"{len(wq)} matches (ratio 0.8)", ""]
