"""The caller-stream contract of the C ABI (sift_mi_set_stream): every kernel
and copy of a call is ordered after the work already enqueued on the caller's
stream, and a call returns after its results are complete.

The late-fill harness.  Every case
  1. allocates its device tensors up front and synchronises the device,
  2. takes a real non-default stream s = torch.cuda.Stream(),
  3. leaves a DECOY in the device input: another valid input of the same
     shape and type (another frame, another descriptor arena, the keypoints of
     another scene), so that a failure of ordering gives a wrong answer and
     never an index out of range; offsets, pair lists and match lists are host
     arguments and the same for both,
  4. enqueues on s a delay (about 50 ms of device time, calibrated once per
     module, no constant), then buf.copy_(real, non_blocking=True) from a
     device tensor, then an event `filled`,
  5. enters the library at once on a context that had set_stream(s).
and asserts (a) `filled` is still pending right before the library call: the
producer had not run when the library was entered (a case whose producer had
finished fails; it neither passes nor skips); (b) the result is the real
input's; (c) beforehand, that the decoy's expected result differs from it.

A context is warmed up with a call on the decoy before the late fill: the first
call of a kind sizes buffers and waits for the stream on the host while it
does, which would order the call by accident.

What (b) compares with: the oracle (extraction), match_ref (matching), the
JPEG restatement; for verification, guided matching, tracks and pair proposal
the same entry point on a second context on its own stream with synchronously
uploaded input -- their agreement with their restatements is held by their own
test files, this file is about order only."""
import functools

import numpy as np
import pytest

import epipolar_ref as E
import jpeg_streams as J
import match_ref
import pairs_ref as R
import tracks_ref as T
import verify_ref as V
from test_gpu_jpeg_streams import reference  # noqa: F401  (the module-scoped fixture of the restatement's luma)
from test_gpu_match_guided import PAIRS as GUIDED_PAIRS
from test_gpu_match_guided import _arena_kps, _arena_models
from test_gpu_pairs import LENS12
from test_gpu_parity import TOL_ANGLE, TOL_RESP, TOL_XY, assert_parity
from test_gpu_tracks import _raw as _tracks_raw

pytestmark = pytest.mark.gpu

W, H = 160, 120
TARGET_MS = 50.0
FILL = 0xA5


# ---- the harness ------------------------------------------------------------------
def _timed(torch, s, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        a.record()
        fn()
        b.record()
    b.synchronize()
    return a.elapsed_time(b)


@pytest.fixture(scope="module")
def delay():
    """A callable that enqueues about TARGET_MS of device time on the current
    torch stream: torch.cuda._sleep with a cycle count calibrated here with
    events, or a chain of matmuls where this torch has no _sleep."""
    import torch
    s = torch.cuda.Stream()
    if hasattr(torch.cuda, "_sleep"):
        unit, n = (lambda k: torch.cuda._sleep(int(k))), 1_000_000
    else:
        x = torch.randn(2048, 2048, device="cuda")

        def unit(k):
            y = x
            for _ in range(int(k)):
                y = y @ x
        n = 4
    _timed(torch, s, lambda: unit(n))  # (first launch: module load)
    for _ in range(12):
        ms = _timed(torch, s, lambda: unit(n))
        if ms >= 5.0:
            break
        n *= 4
    n = max(1, int(n * TARGET_MS / ms))
    fn = lambda: unit(n)  # noqa: E731
    measured = min(_timed(torch, s, fn) for _ in range(2))
    print(f"\nlate-fill delay: {measured:.1f} ms of device time (calibrated count {n})")
    assert 0.5 * TARGET_MS <= measured <= 4 * TARGET_MS, measured
    return fn


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _late(s, delay, fills, call):
    """Steps 4 and 5 and assertion (a): the delay, the fills and the event on
    s, then `call` with no host synchronisation in between."""
    import torch
    with torch.cuda.stream(s):
        delay()
        for buf, real in fills:
            if real is None:
                buf.fill_(FILL)
            else:
                buf.copy_(real, non_blocking=True)
        filled = torch.cuda.Event()
        filled.record(s)
    pending = not filled.query()
    out = call()
    assert pending, "(a) the producer had finished before the library was entered: this run tested no order"
    return out


class _Ctx:
    """A fresh context on torch stream s (None: its own stream), closed before the stream goes away."""

    def __init__(self, pkg, s=None):
        self.pkg, self.s = pkg, s

    def __enter__(self):
        self.c = self.pkg.Context(0, self.pkg.OpenCVProcessing)
        if self.s is not None:
            self.c.set_stream(self.s.cuda_stream)
        return self.c

    def __exit__(self, *exc):
        self.c.close()
        return False


def _sync():
    import torch
    torch.cuda.synchronize()


# ---- extraction ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frame(w, h, seed):
    import synth
    f = synth.frame(w, h, seed)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _want(w, h, seed, limit=None):
    """The oracle's (keypoints, descriptors, emission table) of _frame(w, h, seed), computed once."""
    import oracle
    kw = {} if limit is None else {"features_limit": limit}
    out = oracle.sift(_frame(w, h, seed), internal=True, **kw)
    for a in out:
        a.setflags(write=False)
    return out


def _differ(a, b):
    return len(a[0]) != len(b[0]) or not np.array_equal(a[0], b[0])


def _one(c, buf, limit=None, fetch=True):
    h, w = buf.shape
    return c.sift_batch_device(buf.data_ptr(), 1, w, h, buf.stride(0), buf.numel(), features_limit=limit, fetch=fetch)


@pytest.mark.parametrize("limit", [None, 40])
def test_one_frame(pkg, oracle, synth, delay, limit):
    """The one-chunk path: descriptors on the aux stream, the ordering stage
    on lane 1's stream, both forked from the caller's."""
    import torch
    want, other = _want(W, H, 1, limit), _want(W, H, 2, limit)
    assert _differ(want, other) and len(_want(W, H, 1)[0]) > 40 and len(_want(W, H, 2)[0]) > 40  # (c); the limit cuts
    buf, real = _dev(_frame(W, H, 2)), _dev(_frame(W, H, 1))
    _sync()
    s = torch.cuda.Stream()
    with _Ctx(pkg, s) as c:
        _, warm = _one(c, buf, limit)
        assert_parity(pkg, warm, *other)
        _, res = _late(s, delay, [(buf, real)], lambda: _one(c, buf, limit))
        assert_parity(pkg, res, *want)  # (b)


def _assert_rows(kp, desc, kp_o, desc_o):
    """assert_parity's bounds on keypoint rows and descriptors (the device
    arena of a fetch=False call carries no emission keys; the rows' order is
    still held, to 1e-4 px)."""
    assert len(kp) == len(kp_o), (len(kp), len(kp_o))
    d = np.abs(kp - kp_o)
    assert d[:, :3].max() <= TOL_XY and d[:, 4].max() <= TOL_RESP, d.max(0)
    assert np.abs(((kp[:, 3] - kp_o[:, 3]) + 180.0) % 360.0 - 180.0).max() <= TOL_ANGLE
    dd = np.abs(desc.astype(np.int32) - desc_o.astype(np.int32))
    assert dd.max() <= 1 and (dd == 0).mean() >= 0.99, (dd.max(), (dd == 0).mean())


@pytest.mark.parametrize("lanes", [2, 1])
def test_chunked_batch(pkg, oracle, synth, delay, lanes):
    """Five frames in chunks of two: with two lanes, lane 1 is forked from the
    caller's stream and joined back into it.  The results stay on the device
    and are read on the caller's stream, synchronised only after the copy to
    the host is enqueued."""
    import shard
    import torch
    n = 5
    wants = [_want(W, H, 10 + i) for i in range(n)]
    assert all(_differ(wants[i], _want(W, H, 20 + i)) for i in range(n))  # (c), frame by frame
    buf = _dev(np.stack([_frame(W, H, 20 + i) for i in range(n)]))
    real = _dev(np.stack([_frame(W, H, 10 + i) for i in range(n)]))
    _sync()
    s = torch.cuda.Stream()

    def call(c):
        return c.sift_batch_device(buf.data_ptr(), n, W, H, buf.stride(1), buf.stride(0), fetch=False)[0]

    with _Ctx(pkg, s) as c:
        c.set_chunk(2)
        c.set_pipeline_lanes(lanes)
        call(c)
        offs = _late(s, delay, [(buf, real)], lambda: call(c))
        kp_t, desc_t = shard.device_results(c)
        hk = torch.empty(kp_t.shape, dtype=kp_t.dtype, pin_memory=True)
        hd = torch.empty(desc_t.shape, dtype=desc_t.dtype, pin_memory=True)
        with torch.cuda.stream(s):
            hk.copy_(kp_t, non_blocking=True)
            hd.copy_(desc_t, non_blocking=True)
        s.synchronize()
        kp, desc = hk.numpy().copy(), hd.numpy().copy()
    assert [int(offs[i + 1] - offs[i]) for i in range(n)] == [len(w[0]) for w in wants]
    for i, w in enumerate(wants):
        _assert_rows(kp[offs[i]:offs[i + 1]], desc[offs[i]:offs[i + 1]], w[0], w[1])


def test_graph_replay(pkg, oracle, synth, delay):
    """Path option graph = 1 on a caller stream: three identical one-frame
    calls on one buffer (first sighting, capture, replay), a different frame
    late-filled before each; the delay and the fill are on the stream before
    the library begins its capture.  Each call gives the frame it was handed.
    (The context has seen all three frames before, so its stage bounds -- part
    of the graph's key -- no longer move; total_ms counts graph launches only
    in the two-lane mode.)"""
    import torch
    seeds = [31, 32, 33]
    frames = [_dev(_frame(W, H, k)) for k in seeds]
    buf = torch.empty_like(frames[0])
    _sync()
    s = torch.cuda.Stream()
    with _Ctx(pkg, s) as c:
        for f in frames:
            buf.copy_(f)
            _sync()
            _one(c, buf)
        c.set_path_option("graph", 1)
        c.reset_stats()
        launched = []
        for i, k in enumerate(seeds):
            assert _differ(_want(W, H, k), _want(W, H, seeds[i - 1]))  # (c): the buffer holds the frame before
            _, res = _late(s, delay, [(buf, frames[i])], lambda: _one(c, buf))
            assert_parity(pkg, res, *_want(W, H, k))
            launched.append(c.stats()["total_ms"] > 0)
        assert launched == [False, True, True], launched  # the second call captured and launched a graph


def test_switching_streams(pkg, ctx, oracle, synth, delay):
    """One context with graph = 1: a 96x64 frame on s1, then 160x120 frames on
    s2 five times (the buffers grow after the change of stream; two frames
    alternate, so the stage bounds settle and the later calls capture and
    replay: total_ms counts graph launches), on s1 (the same key but for the
    stream, so a first sighting again), on its own stream, and on s1 again.
    Every call on a caller stream gets a late fill on that stream.  What this
    pins: the order on the stream in force after every change, the grow path
    of reserve_chunk after a change, and the re-sighting.  It does not pin the
    stream field of the graph's key: a replay is launched on the stream in
    force whatever stream was captured."""
    import torch
    small = _dev(_frame(96, 64, 41))
    frames = {k: _dev(_frame(W, H, k)) for k in (42, 43)}
    bs, bl = _dev(_frame(96, 64, 40)), _dev(_frame(W, H, 43))
    _sync()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    assert _differ(_want(96, 64, 41), _want(96, 64, 40)) and _differ(_want(W, H, 42), _want(W, H, 43))  # (c)
    with _Ctx(pkg) as c:
        c.set_path_option("graph", 1)
        c.set_stream(s1.cuda_stream)
        _, res = _late(s1, delay, [(bs, small)], lambda: _one(c, bs))
        assert_parity(pkg, res, *_want(96, 64, 41))
        for i, s in enumerate([s2, s2, s2, s2, s2, s1, None, s1]):
            k = 42 + i % 2  # the buffer holds the other frame
            c.set_stream(None if s is None else s.cuda_stream)
            if s is None:
                bl.copy_(frames[k])
                _sync()
                _, res = _one(c, bl)
                assert res == _one(ctx, bl)[1]  # its own stream again: what the fixture context gives
            else:
                _, res = _late(s, delay, [(bl, frames[k])], lambda: _one(c, bl))
            assert_parity(pkg, res, *_want(W, H, k))
            if i == 4:
                assert c.stats()["total_ms"] > 0  # a graph was launched on s2


@pytest.mark.parametrize("null", [None, 0])
def test_set_stream_null_restores_the_own_stream(pkg, ctx, synth, delay, null):
    import torch
    buf, real = _dev(_frame(W, H, 2)), _dev(_frame(W, H, 1))
    _sync()
    s = torch.cuda.Stream()
    with _Ctx(pkg, s) as c:
        _one(c, buf)
        _, res = _late(s, delay, [(buf, real)], lambda: _one(c, buf))
        want = _one(ctx, buf)[1]
        assert res == want and np.array_equal(res.keys, want.keys)
        c.set_stream(null)
        for f in (2, 1):
            buf.copy_(_dev(_frame(W, H, f)))
            _sync()
            got, want = _one(c, buf)[1], _one(ctx, buf)[1]
            assert got == want and np.array_equal(got.keys, want.keys) and len(got) > 0


# ---- matching -----------------------------------------------------------------------------
SEGS = [40, 129, 300]
SEG_PAIRS = [(0, 1), (1, 2), (2, 1), (1, 0), (0, 2), (1, 1)]


def _match_arena(seed):
    """Three segments; a third of each shorter one's rows are noisy copies of rows of the next."""
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(SEGS)]).astype(np.int64)
    rows = rng.integers(0, 256, (int(offs[-1]), 128), dtype=np.uint8)
    for a in range(len(SEGS) - 1):
        k = SEGS[a] // 3
        src = offs[a + 1] + rng.permutation(SEGS[a + 1])[:k]
        noise = rng.integers(-3, 4, (k, 128))
        rows[offs[a]:offs[a] + k] = np.clip(rows[src].astype(np.int64) + noise, 0, 255).astype(np.uint8)
    return rows, offs


def _same_matches(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


def test_match_pairs_device(pkg, delay):
    import torch
    (rows, offs), (decoy, _) = _match_arena(1), _match_arena(2)
    seg = lambda r, k: r[offs[k]:offs[k + 1]]  # noqa: E731
    want = [match_ref.match(seg(rows, a), seg(rows, b), 0.8, True) for a, b in SEG_PAIRS]
    other = [match_ref.match(seg(decoy, a), seg(decoy, b), 0.8, True) for a, b in SEG_PAIRS]
    assert all(len(w[0]) >= 8 for w in want[:4])  # the planted thirds, less those the later plants overwrote
    assert not all(_same_matches(w, o) for w, o in zip(want, other))  # (c)
    buf, real = _dev(decoy), _dev(rows)
    _sync()
    s = torch.cuda.Stream()
    call = lambda c: c.match_pairs_device(buf.data_ptr(), offs, SEG_PAIRS, ratio=0.8, cross_check=True)  # noqa: E731
    with _Ctx(pkg, s) as c:
        assert all(_same_matches(g, o) for g, o in zip(call(c), other))
        got = _late(s, delay, [(buf, real)], lambda: call(c))
    for p, (g, w) in enumerate(zip(got, want)):
        assert _same_matches(g, w), (SEG_PAIRS[p], len(g[0]), len(w[0]))


# ---- verification, guided matching, tracks, pair proposal: against a second context --------
def _same_models(a, b):
    return len(a) == len(b) and all(
        np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32)) and np.array_equal(x[1], y[1]) and x[2] == y[2]
        for x, y in zip(a, b))


@pytest.mark.parametrize("model", ["homography", "fundamental"])
def test_verify_pairs_device(pkg, delay, model):
    import torch
    mod = V if model == "homography" else E
    kps, offs, pairs, matches, _ = mod.segments()
    decoy = mod.segments(seed=22)[0]  # another scene in the same segments
    assert decoy.shape == kps.shape and np.isfinite(decoy).all()
    buf, real, sync_real, sync_decoy = _dev(decoy), _dev(kps), _dev(kps), _dev(decoy)
    _sync()
    s = torch.cuda.Stream()

    def call(c, t):
        return c.verify_pairs_device(t.data_ptr(), offs, pairs, matches, threshold=2.0, iterations=300, seed=5,
                                     refit_rounds=1, model=model)

    with _Ctx(pkg) as c2, _Ctx(pkg, s) as c:
        want, other = call(c2, sync_real), call(c2, sync_decoy)
        assert not _same_models(want, other) and sum(w[2]["n_inliers"] for w in want) > 500  # (c)
        assert _same_models(call(c, buf), other)
        got = _late(s, delay, [(buf, real)], lambda: call(c, buf))
        assert _same_models(got, want)  # (b)


@pytest.mark.parametrize("model", ["homography", "fundamental"])
def test_match_pairs_guided_device(pkg, delay, model):
    import torch
    rows, offs = match_ref.segment_arena()
    kps = _arena_kps(offs)
    rng = np.random.default_rng(8)
    decoy_rows = rng.integers(0, 256, rows.shape, dtype=np.uint8)
    decoy_kps = kps.copy()
    decoy_kps[:, :2] = kps[rng.permutation(len(kps)), :2]  # the same places, other rows on them
    models = _arena_models(model)
    bd, bk = _dev(decoy_rows), _dev(decoy_kps)
    rd, rk, dd, dk = _dev(rows), _dev(kps), _dev(decoy_rows), _dev(decoy_kps)
    _sync()
    s = torch.cuda.Stream()

    def call(c, d, k):
        return c.match_pairs_guided_device(d.data_ptr(), k.data_ptr(), offs, GUIDED_PAIRS, models, threshold=3.0,
                                           model=model, ratio=0.8, cross_check=True)

    same = lambda a, b: all(_same_matches(x, y) for x, y in zip(a, b))  # noqa: E731
    with _Ctx(pkg) as c2, _Ctx(pkg, s) as c:
        want, other = call(c2, rd, rk), call(c2, dd, dk)
        assert not same(want, other) and sum(len(w[0]) for w in want) > 0  # (c)
        # either arena alone must matter: descriptors of the real input on the decoy's keypoints and the reverse
        assert not same(want, call(c2, rd, dk)) and not same(want, call(c2, dd, rk))
        assert same(call(c, bd, bk), other)
        got = _late(s, delay, [(bd, rd), (bk, rk)], lambda: call(c, bd, bk))
        assert same(got, want)  # (b)


def test_build_tracks_device(pkg, delay):
    """The keep mask, like the matches, is a host argument of
    sift_mi_build_tracks_device: only the keypoints are late-filled."""
    import torch
    g = T.random_graph(T.SEG_LENS, 16, 0.3, 5, keep_share=0.8)
    n = int(g["offsets"][-1])
    kps, decoy = T.keypoints(n, seed=1), T.keypoints(n, seed=2)
    buf, real, sync_real, sync_decoy = _dev(decoy), _dev(kps), _dev(kps), _dev(decoy)
    _sync()
    s = torch.cuda.Stream()

    def call(c, t):
        rc, out = _tracks_raw(pkg, c, t.data_ptr(), g)
        assert rc == 0, pkg.lib().sift_mi_last_error()
        return out

    with _Ctx(pkg) as c2, _Ctx(pkg, s) as c:
        want, other = call(c2, sync_real), call(c2, sync_decoy)
        assert len(want["obs"]) > 50 and not T.equal(want, other)  # (c)
        assert T.equal(call(c, buf), other)
        got = _late(s, delay, [(buf, real)], lambda: call(c, buf))
        assert T.equal(got, want)  # (b)


def test_propose_pairs_device(pkg, delay):
    import torch
    (desc, kps, offs), (d_desc, d_kps, d_offs) = R.arena(LENS12, seed=12), R.arena(LENS12, seed=13)
    assert np.array_equal(offs, d_offs)
    bd, bk = _dev(d_desc), _dev(d_kps)
    rd, rk, dd, dk = _dev(desc), _dev(kps), _dev(d_desc), _dev(d_kps)
    _sync()
    s = torch.cuda.Stream()

    def call(c, d, k):
        return c.propose_pairs_device(d.data_ptr(), k.data_ptr(), offs, 64, 0.8, 8, 0)

    same = lambda a, b: a[0] == b[0] and np.array_equal(a[1], b[1])  # noqa: E731
    with _Ctx(pkg) as c2, _Ctx(pkg, s) as c:
        want, other = call(c2, rd, rk), call(c2, dd, dk)
        assert len(want[0]) >= 3 and not same(want, other)  # (c)
        assert not same(want, call(c2, rd, dk)) and not same(want, call(c2, dd, rk))  # either arena matters
        assert same(call(c, bd, bk), other)
        got = _late(s, delay, [(bd, rd), (bk, rk)], lambda: call(c, bd, bk))
        assert same(got, want)  # (b)


# ---- JPEG: write after write ------------------------------------------------------------------
def _waw_expected(ref, shape, w, h):
    want = np.full(shape, FILL, np.uint8)
    want[..., :h, :w] = ref
    return want


@pytest.mark.parametrize("name", [J.BATCH[0], J.BATCH[5]])
def test_decode_jpeg_device_after_a_fill(pkg, reference, delay, name):
    """On s: the delay, out.fill_(0xA5), then the decode into `out`, whose rows
    are wider than the image.  A decode that did not wait for the fill is
    overwritten by it: 0xA5 everywhere."""
    import torch
    sp, data = J.spec(name), J.stream(name)[0]
    ref = reference(name)
    assert (ref != FILL).mean() > 0.5  # (c): the image is not the fill
    out = torch.zeros((sp.h + 2, sp.w + 8), dtype=torch.uint8, device="cuda")
    scratch = torch.zeros_like(out)
    _sync()
    s = torch.cuda.Stream()
    with _Ctx(pkg, s) as c:
        c.decode_jpeg_device(data, scratch.data_ptr(), scratch.stride(0))
        _late(s, delay, [(out, None)], lambda: c.decode_jpeg_device(data, out.data_ptr(), out.stride(0)))
        s.synchronize()
        got = out.cpu().numpy()
    assert np.array_equal(got, _waw_expected(ref, got.shape, sp.w, sp.h))


@pytest.mark.parametrize("threads", [1, 4])
def test_decode_jpeg_batch_device_after_a_fill(pkg, reference, delay, threads):
    """The same for the batch decode, whose "a caller stream is used as is"
    branch runs the reconstruction on s itself; 20 frames are two of its
    chunks."""
    import torch
    names = [J.BATCH[i % len(J.BATCH)] for i in range(20)]
    sp = J.spec(names[0])
    datas = [J.stream(n)[0] for n in names]
    ref = np.stack([reference(n) for n in names])
    assert (ref != FILL).mean() > 0.5  # (c)
    out = torch.zeros((len(names), sp.h, sp.w + 8), dtype=torch.uint8, device="cuda")
    scratch = torch.zeros_like(out)
    _sync()
    s = torch.cuda.Stream()

    def call(c, t):
        c.decode_jpeg_batch_device(datas, t.data_ptr(), t.stride(0), t.stride(1), threads=threads)

    with _Ctx(pkg, s) as c:
        call(c, scratch)
        _late(s, delay, [(out, None)], lambda: call(c, out))
        s.synchronize()
        got = out.cpu().numpy()
    assert np.array_equal(got, _waw_expected(ref, got.shape, sp.w, sp.h))
