"""The call-sequence contract of the C ABI on a long-lived context.

A consumer creates one context and calls it for hours with changing shapes,
batch sizes, limits and modes; sift_mi_ctx carries a plan and two arenas,
grow-only buffers, high-water marks, the result state (result_state.h) and a
graph cache from call to call.  Three parts, everything bit-exact
(SiftResult.__eq__ and np.array_equal on the keys; no tolerance):

  (a) the ABI state on the device: scripted sequences of raw ctypes calls on a
      fresh context; every return-code class is tests/call_model.py's, and
      wherever fetch / device_results succeeds the rows are those of the
      producing call made alone on a fresh context.  The sequences of the four
      defects the result-state header fixed are among them (4b, a precompute
      that fails after the plan was replaced, needs a failed allocation and is
      left to tests/test_host_result_state.py);
  (b) one context per profile walks ~40 calls (sizes down, up and transposed,
      chunk sizes, dense / empty / dense, limits, exact descriptors, octave
      caps, lanes, row bands, device-kept batches, precompute between batches);
      every result equals the same call on a context made for it, three steps
      also go through assert_parity against the oracle, and after a step that
      follows a larger shape the arena's planes equal the oracle's pyramid;
  (c) the graph cache (path option graph = 1) under interleaved calls of two
      batch sizes and two frame sizes on one context.

Frames are kernel_shapes.noise (no stale or shifted row of a plane can cancel),
patterns.make("white") is the frame without a keypoint.  SHAPES are the smallest
that reach different kernel families; test_shapes_reach_the_kernel_families
states which, from kernel_shapes.dispatch.
"""
import ctypes

import numpy as np
import pytest

import call_model as M
import kernel_shapes as K
import patterns

gpu = pytest.mark.gpu

ESTATE, EINVAL = -6, -1
SHAPES = [(96, 64), (64, 96), (200, 150), (320, 240)]
TAIL_ONLY = (48, 32)  # every octave in k_octave_tail
WHITE = patterns.REGISTRY["white"][1], patterns.REGISTRY["white"][0]  # (w, h) = (161, 97)
FRESH = {"contexts": 0}  # fresh contexts this module made (printed by the tests)


def _frame(w, h, k=0, kind="noise"):
    """Frame k of a (w, h) batch: the shape's noise frame rolled by 7 k columns
    (still noise, different from its neighbours), or the flat white frame."""
    if kind == "white":
        assert (w, h) == WHITE
        return patterns.make("white")
    return np.ascontiguousarray(np.roll(K.noise(w, h), 7 * k, axis=1))


def test_shapes_reach_the_kernel_families():
    """What the set reaches, by the dispatch mirror, in both profiles.  No frame
    of the four sizes the walk was given is tail-only from octave 0 (their
    octave 0 is above the tail's LDS capacity): 96 x 64 and 64 x 96 run octave 0
    with per-blur launches and every other octave in the tail launch, the first
    with the seed pair and the second without; TAIL_ONLY adds the frame whose
    octaves all run in the tail.  The fused blur-5 + scan pass takes test-sized
    frames only under fused_detect = 2, which the walk sets for two steps."""
    for p in K.PROFILES:
        assert K.dispatch(*TAIL_ONLY, p)[0] == 0  # the tail-only family
        for w, h in SHAPES[:2]:
            assert K.dispatch(w, h, p)[0] == 1  # octave 0, then the tail
        assert K.seed_pair_applies(*K.octave_sizes(96, 64)[0]) and not K.seed_pair_applies(*K.octave_sizes(64, 96)[0])
        for w, h in SHAPES[2:]:
            sizes, o_tail = K.octave_sizes(w, h), K.dispatch(w, h, p)[0]
            assert K.seed_pair_applies(*sizes[0])  # seed pair
            assert o_tail >= 2 and K.pair_applies(*sizes[1])  # pair blur below the tail, beyond octave 0
            assert {f[5] for f in K.blur_families(w, h, p)} == {"strip"}  # strip blurs 4, 5
            assert K.fused_octaves(w, h, p, {"fused_detect": 2}) == list(range(o_tail))  # fused scan
        assert K.dispatch(320, 240, p)[0] == 3 and K.dispatch(200, 150, p)[0] == 2
    assert SHAPES[0][0] * SHAPES[0][1] == SHAPES[1][0] * SHAPES[1][1] and SHAPES[0][0] != SHAPES[1][0]


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def _processing(pkg, profile):
    return pkg.OpenCVProcessing if profile == 0 else pkg.ImageprocProcessing


def _fresh(pkg, profile=0):
    FRESH["contexts"] += 1
    return pkg.Context(0, _processing(pkg, profile))


_hip = None


def _copy_back(kp_ptr, desc_ptr, n):
    """n device rows as host arrays (hipMemcpy, as test_gpu_configs._device_results)."""
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    kp = np.empty((n, 5), np.float32)
    desc = np.empty((n, 128), np.uint8)
    if n:
        assert kp_ptr and desc_ptr
        assert _hip.hipMemcpy(kp.ctypes.data, kp_ptr, kp.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        assert _hip.hipMemcpy(desc.ctypes.data, desc_ptr, desc.nbytes, 2) == 0
    return kp, desc


def _same(a, b, what):
    """Two lists of SiftResult (keys None where a call has none): bit-equal."""
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y), (what, i, len(x), len(y))
        assert x == y, (what, i)
        if x.keys is not None and y.keys is not None:
            assert np.array_equal(x.keys, y.keys), (what, i)


# ---------------------------------------------------------------------------
# (a) the ABI state on the device
# ---------------------------------------------------------------------------
class _Abi:
    """Raw calls on one context; every method returns the status code."""

    def __init__(self, pkg, w, h):
        import torch
        self.torch, self.pkg, self.L = torch, pkg, pkg.lib()
        self.ctx = _fresh(pkg)
        self.h = self.ctx._h
        self.w, self.hh = w, h
        self.L.sift_mi_set_chunk(self.h, 1)  # one frame: one chunk; three frames: three chunks
        self.pre = None  # the frame of the last successful precompute
        self.tensors = []

    def close(self):
        self.ctx.close()

    def frames(self, pos, one_chunk):
        return np.stack([_frame(self.w, self.hh, 3 * pos + k) for k in range(1 if one_chunk else 3)])

    def call(self, pos, letter):
        """Run call `letter` (call_model.ALPHABET) as the pos-th of its script: (status, rows or None)."""
        L, h = self.L, self.h
        name, outcome, arg = M.ALPHABET[letter]
        assert outcome != "late"  # needs a failed allocation: the stand-alone program's part
        sz, u32 = ctypes.c_size_t, ctypes.c_uint32
        if name in ("extract", "extract_device"):
            f = self.frames(pos, arg)
            n = len(f)
            offs = (sz * (n + 1))()
            limit = -1
            if outcome == "bad":  # features_limit under row bands, refused on both entry paths
                assert L.sift_mi_set_row_band(h, 0, 2) == 0
                limit = 5
            if name == "extract":
                ptrs = (ctypes.c_void_p * n)(*[f[i].ctypes.data for i in range(n)])
                rc = L.sift_mi_extract_batch(h, ptrs, n, self.w, self.hh, self.w, limit, offs)
            else:
                t = self.torch.from_numpy(f).cuda()
                self.torch.cuda.synchronize()
                self.tensors.append(t)
                rc = L.sift_mi_extract_batch_device(h, t.data_ptr(), t.stride(0), n, self.w, self.hh, t.stride(1),
                                                    limit, offs)
            assert L.sift_mi_set_row_band(h, 0, 1) == 0
            return rc, None
        if name == "precompute":
            img = _frame(self.w, self.hh, 3 * pos)
            n = sz()
            rc = L.sift_mi_precompute(h, img.ctypes.data, self.w, self.hh, self.w - 1 if outcome == "bad" else self.w,
                                      ctypes.byref(n))
            if rc == 0:
                self.pre = pos
            return rc, None
        if name == "with_precomputed":
            n = sz()
            if outcome == "bad":
                assert L.sift_mi_set_row_band(h, 0, 2) == 0
            rc = L.sift_mi_sift_with_precomputed(h, 5 if outcome == "bad" else -1, ctypes.byref(n))
            assert L.sift_mi_set_row_band(h, 0, 1) == 0
            return rc, None
        if name == "set_keep":
            return L.sift_mi_set_keep_on_device(h, 1 if arg else 0), None
        if name == "set_max_octaves":
            return L.sift_mi_set_max_octaves(h, 0), None
        if name == "read_pyramid":
            a, b = u32(), u32()
            return L.sift_mi_octave_dims(h, 0, ctypes.byref(a), ctypes.byref(b)), None
        if name == "read_batch":
            a, b = u32(), u32()
            return L.sift_mi_batch_octave_dims(h, 0, ctypes.byref(a), ctypes.byref(b)), None
        raise KeyError(name)

    def fetch(self, n):
        """sift_mi_fetch + sift_mi_fetch_keys into arrays of exactly the expected n rows (and a guard row)."""
        kps = np.zeros((n + 1, 5), np.float32)
        desc = np.zeros((n + 1, 128), np.uint8)
        keys = np.zeros(n + 1, np.uint64)
        rc = self.L.sift_mi_fetch(self.h, kps.ctypes.data, desc.ctypes.data, n)
        rc2 = self.L.sift_mi_fetch_keys(self.h, keys.ctypes.data, n)
        assert rc == rc2, (rc, rc2)
        assert not kps[n].any() and not desc[n].any() and not keys[n]
        return rc, (kps[:n], desc[:n], keys[:n])

    def device_results(self, n):
        kp, desc, m = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        rc = self.L.sift_mi_device_results(self.h, ctypes.byref(kp), ctypes.byref(desc), ctypes.byref(m))
        if rc != 0:
            return rc, None
        assert m.value == n, (m.value, n)  # checked before anything is copied
        return rc, _copy_back(kp.value, desc.value, n)


_alone = {}


def _alone_rows(pkg, w, h, pos, letter, pre):
    """(kps, desc, keys) of producing call `letter` at script position pos, made alone on a fresh context."""
    name, _, arg = M.ALPHABET[letter]
    key = (w, h, name, arg, pre if name == "with_precomputed" else pos)
    if key not in _alone:
        c = _fresh(pkg)
        try:
            c.set_chunk(1)
            if name == "with_precomputed":
                r = [c.sift_with_precomputed(c.precompute_images(_frame(w, h, 3 * pre)))]
            else:
                f = np.stack([_frame(w, h, 3 * pos + k) for k in range(1 if arg else 3)])
                if name == "extract":
                    r = c.sift_batch(f)
                else:
                    import torch
                    t = torch.from_numpy(f).cuda()
                    torch.cuda.synchronize()
                    r = [c.sift_batch_device(t.data_ptr(), len(f), w, h, t.stride(1), t.stride(0))[1]]
        finally:
            c.close()
        _alone[key] = (np.concatenate([x.keypoints_array for x in r]), np.concatenate([x.descriptors for x in r]),
                       np.concatenate([x.keys for x in r]))
    return _alone[key]


# word, shape: 4-8 calls each over call_model.ALPHABET (no "late" letters)
SCRIPTS = [
    ("KaFDkF", (96, 64)),     # defect 1: fetch after a host-frame call under keep = 1
    ("KeDaDFeD", (96, 64)),   # defect 2: no stale device pointers after a later host-frame call
    ("KekFDKD", (96, 64)),    # defect 3: no host read of a device-kept result once keep is 0
    ("pstFP", (64, 96)),      # defect 4a: a refused sift_with_precomputed keeps the row count
    ("acFgFB", (64, 96)),     # the same refusal on both extraction entry paths
    ("pPaPsB", (96, 64)),     # an extraction ends the precomputed pyramid
    ("aBMBF", (200, 150)),    # set_max_octaves ends the batch read-back, not the result
    ("psBFpF", (200, 150)),   # precompute ends the result
    ("KfDbDF", (96, 64)),     # several chunks: the device arena, then the host buffers
    ("eFKFeFD", (64, 96)),    # the setting moves; the last result does not
    ("FDPBsaF", (96, 64)),    # nothing to read on a new context
    ("KeqDgDtD", (64, 96)),   # refused calls leave a device result readable
    ("psMsPps", (96, 64)),    # set_max_octaves ends the pyramid
]


def test_scripts_include_the_defect_sequences():
    words = [w for w, _ in SCRIPTS]
    assert all(4 <= len(w) <= 8 for w in words) and len(words) >= 12
    assert not any(M.ALPHABET[ch][1] == "late" for w in words for ch in w)
    # defects 1, 2, 3 and 4a, and after each refused read the result the model still has
    assert words[0] == "KaFDkF" and words[1].startswith("KeDaDF") and words[2].startswith("KekFD")
    assert words[3].startswith("pstF") and "cF" in words[4] and "gF" in words[4]
    for w in words:  # every script's classes, by the model: each has a refusal or a read that succeeds
        classes = [c for c, _, _ in M.run([M.ALPHABET[ch] for ch in w])]
        assert M.OK in classes and (M.ESTATE in classes or M.EINVAL in classes), w


@gpu
@pytest.mark.parametrize("word,shape", SCRIPTS, ids=[w for w, _ in SCRIPTS])
def test_abi_state_on_the_device(pkg, word, shape):
    w, h = shape
    want = M.run([M.ALPHABET[ch] for ch in word])
    abi = _Abi(pkg, w, h)
    produced = {}  # rows number of the model (position + 1) -> (letter, position, precomputed frame)
    reads = 0
    try:
        for pos, ch in enumerate(word):
            cls, n_model, state = want[pos]
            name = M.ALPHABET[ch][0]
            if name in ("fetch", "device_results"):
                letter, ppos, pre = produced[n_model] if cls == M.OK else (None, None, None)
                rows = _alone_rows(pkg, w, h, ppos, letter, pre) if cls == M.OK else None
                n = len(rows[0]) if rows else 0
                rc, got = abi.fetch(n) if name == "fetch" else abi.device_results(n)
                if cls == M.OK:
                    assert n > 0  # noise frames have keypoints: equal rows mean something
                    assert np.array_equal(got[0], rows[0]) and np.array_equal(got[1], rows[1]), (word, pos)
                    if name == "fetch":
                        assert np.array_equal(got[2], rows[2]), (word, pos)
                    reads += 1
            else:
                rc, _ = abi.call(pos, ch)
                if cls == M.OK and name in M.PRODUCING and name != "precompute":
                    produced[pos + 1] = (ch, pos, abi.pre)
            got_cls = {0: M.OK, ESTATE: M.ESTATE, EINVAL: M.EINVAL}.get(rc, rc)
            assert got_cls == cls, (word, pos, ch, rc, pkg.lib().sift_mi_last_error())
    finally:
        abi.close()
    print(f"\nSCRIPT {word} {w}x{h}: {reads} successful reads; fresh contexts so far {FRESH['contexts']}")


# ---------------------------------------------------------------------------
# (b) a long-lived context equals fresh contexts
# ---------------------------------------------------------------------------
DEFAULTS = {"chunk": 0, "exact": 0, "max_octaves": 0, "lanes": 2, "band": (0, 1), "fused_detect": 1}


def _apply(c, name, value):
    if name == "chunk":
        c.set_chunk(value)
    elif name == "exact":
        c.set_exact_descriptors(bool(value))
    elif name == "max_octaves":
        c.set_max_octaves(value)
    elif name == "lanes":
        c.set_pipeline_lanes(value)
    elif name == "band":
        c.set_row_band(*value)
    elif name == "fused_detect":
        c.set_path_option("fused_detect", value)
    else:
        raise KeyError(name)


def _run_call(pkg, c, call):
    """One call of the walk on context c: a list of SiftResult (device-kept rows
    read through device_results, one SiftResult per frame, keys None)."""
    kind, (w, h), kinds, limit = call
    frames = np.stack([_frame(w, h, k, kd) for k, kd in enumerate(kinds)])
    if kind == "sift":
        return [c.sift(frames[0], features_limit=limit)]
    if kind == "batch":
        return c.sift_batch(frames, features_limit=limit)
    if kind == "precomputed":
        pre = c.precompute_images(frames[0])
        return [c.sift_with_precomputed(pre, features_limit=limit)]
    import torch
    t = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    n = len(frames)
    offs, res = c.sift_batch_device(t.data_ptr(), n, w, h, t.stride(1), t.stride(0), features_limit=limit,
                                    fetch=kind == "device")
    if kind == "device":
        kp, desc, keys = res.keypoints_array, res.descriptors, res.keys
    else:
        assert kind == "device_kept" and res is None
        kp_ptr, desc_ptr, m = c.device_results()
        assert m == int(offs[-1])
        kp, desc = _copy_back(kp_ptr, desc_ptr, m)
        keys = None
    return [pkg.SiftResult(kp[offs[i]:offs[i + 1]], desc[offs[i]:offs[i + 1]],
                           None if keys is None else keys[offs[i]:offs[i + 1]]) for i in range(n)]


N3, N5 = ("noise",) * 3, ("noise",) * 5
DEW = ("noise", "white", "noise")
S200, S320 = (200, 150), (320, 240)
# (settings changed before the call, call, note): the walk, in order
WALK = [
    ({}, ("sift", S320, ("noise",), None), "parity"),
    ({}, ("sift", (96, 64), ("noise",), None), "size down"),
    ({}, ("sift", (64, 96), ("noise",), None), "transposed"),
    ({}, ("sift", S200, ("noise",), None), "size up"),
    ({}, ("sift", S320, ("noise",), None), "size up, as at first"),
    ({}, ("sift", TAIL_ONLY, ("noise",), None), "tail only"),
    ({"chunk": 1}, ("batch", S200, N5, None), "chunk 1"),
    ({"chunk": 5}, ("batch", S200, N5, None), "chunk 5: the arenas grow, the marks stay"),
    ({"chunk": 2}, ("batch", S200, N5, None), "chunk 2, parity"),
    ({"chunk": 5}, ("batch", S200, N5, None), "chunk 5 again"),
    ({"chunk": 0}, ("batch", S200, ("noise",), None), "n 1"),
    ({}, ("batch", S200, N5, None), "n 5"),
    ({}, ("batch", S200, ("noise",) * 2, None), "n 2"),
    ({}, ("batch", S200, N5, None), "n 5 again"),
    ({}, ("sift", WHITE, ("noise",), None), "dense"),
    ({}, ("sift", WHITE, ("white",), None), "empty: a whole call without a keypoint"),
    ({}, ("sift", WHITE, ("noise",), None), "dense again: bounds from the marks"),
    ({}, ("batch", WHITE, DEW, None), "an empty frame inside one chunk"),
    ({"chunk": 1}, ("batch", WHITE, DEW, None), "an empty frame as a whole chunk"),
    ({"chunk": 0}, ("sift", S200, ("noise",), 3), "limit 3, parity"),
    ({}, ("sift", S200, ("noise",), 0), "limit 0"),
    ({}, ("sift", S200, ("noise",), None), "limit None"),
    ({"exact": 1}, ("sift", S200, ("noise",), None), "exact descriptors on"),
    ({"exact": 0}, ("sift", S200, ("noise",), None), "exact descriptors off"),
    ({"max_octaves": 2}, ("sift", S200, ("noise",), None), "max_octaves 2"),
    ({"max_octaves": 0}, ("sift", S200, ("noise",), None), "max_octaves 0"),
    ({"fused_detect": 2}, ("sift", S320, ("noise",), None), "the fused blur 5 + scan pass"),
    ({}, ("batch", S200, N3, None), "the fused pass, three frames, after a larger shape"),
    ({"fused_detect": 1}, ("sift", S200, ("noise",), None), "fused_detect as by default"),
    ({"chunk": 2, "lanes": 1}, ("batch", S200, N5, None), "lanes 1"),
    ({"lanes": 2}, ("batch", S200, N5, None), "lanes 2"),
    ({"chunk": 0, "band": (1, 2)}, ("sift", S200, ("noise",), None), "row band 1 of 2"),
    ({"band": (0, 1)}, ("sift", S200, ("noise",), None), "whole"),
    ({}, ("device_kept", S200, N3, None), "a device-kept batch"),
    ({}, ("sift", (96, 64), ("noise",), None), "a host call between them"),
    ({}, ("device_kept", S200, N3, None), "a device-kept batch again"),
    ({}, ("device", S200, N3, None), "the same frames, fetched"),
    ({}, ("batch", S200, ("noise",) * 2, None), "a batch"),
    ({}, ("precomputed", S200, ("noise",), None), "precompute + sift_with_precomputed"),
    ({}, ("batch", S200, ("noise",) * 2, None), "a batch after it"),
]
PARITY_STEPS = (0, 8, 19)


def test_walk_covers_the_listed_state():
    calls = [c for _, c, _ in WALK]
    assert [c[1] for c in calls[:5]] == [S320, (96, 64), (64, 96), S200, S320]
    assert [s.get("chunk") for s, _, _ in WALK[6:10]] == [1, 5, 2, 5]
    assert [len(c[2]) for c in calls[10:14]] == [1, 5, 2, 5]
    assert [c[3] for c in calls[19:22]] == [3, 0, None]
    assert sum(c[0] == "device_kept" for c in calls) == 2 and any(c[0] == "precomputed" for c in calls)
    assert all(WALK[i][2].endswith("parity") for i in PARITY_STEPS)
    assert {c[1] for c in calls} >= set(SHAPES)


@gpu
@pytest.mark.parametrize("profile", [0, 1])
def test_long_lived_context_equals_fresh_contexts(pkg, oracle, profile):
    from test_gpu_parity import assert_parity
    fresh0 = FRESH["contexts"]
    memo = {}

    def alone(settings, call):
        key = (tuple(sorted(settings.items())), call)
        if key not in memo:
            c = _fresh(pkg, profile)
            try:
                for k in DEFAULTS:  # a fixed order
                    if settings[k] != DEFAULTS[k]:
                        _apply(c, k, settings[k])
                memo[key] = _run_call(pkg, c, call)
            finally:
                c.close()
        return memo[key]

    c = pkg.Context(0, _processing(pkg, profile))
    settings = dict(DEFAULTS)
    prev_px = 0
    readbacks = 0
    try:
        for step, (change, call, note) in enumerate(WALK):
            for k, v in change.items():
                _apply(c, k, v)
                settings[k] = v
            kind, (w, h), kinds, limit = call
            got = _run_call(pkg, c, call)
            _same(got, alone(settings, call), (step, note))
            for r, kd in zip(got, kinds):  # equal results that are not all empty
                assert (len(r) == 0) == (kd == "white" or limit == 0), (step, note, len(r))
            if step in PARITY_STEPS:  # "equal" is not "equally wrong"
                f = len(kinds) - 2 if len(kinds) > 1 else 0
                kp_o, desc_o, ext_o = oracle.sift(_frame(w, h, f, kinds[f]), features_limit=limit, profile=profile,
                                                  internal=True)
                assert len(kp_o) > 0
                assert_parity(pkg, got[f], kp_o, desc_o, ext_o)
            if kind == "precomputed":  # equals sift() of the same frame
                _same(got, alone(settings, ("sift", (w, h), kinds, limit)), (step, note, "sift"))
            if note == "whole":  # after the band reset: the whole frame
                _same(got, alone(DEFAULTS, call), (step, note, "defaults"))
                assert len(got[0]) > len(alone({**DEFAULTS, "band": (1, 2)}, call)[0]) > 0
            one_chunk = kind != "precomputed" and (len(kinds) == 1 or settings["chunk"] in (0, 5)) \
                and settings["band"] == (0, 1)
            if one_chunk and w * h < prev_px and settings["max_octaves"] == 0:
                # no plane of the larger plan survived the re-plan
                for f in {0, len(kinds) - 1}:
                    opy = oracle.Pyramid(_frame(w, h, f, kinds[f]), profile)
                    for o in (0, opy.n_octaves - 1):
                        assert np.array_equal(c.read_batch_scale_space(f, o), opy.scale_space(o)), (step, note, f, o)
                readbacks += 1
            prev_px = w * h
        # after an extraction call the earlier PrecomputedImages is refused at the ABI
        n, a, b = ctypes.c_size_t(), ctypes.c_uint32(), ctypes.c_uint32()
        L = pkg.lib()
        assert L.sift_mi_sift_with_precomputed(c._h, -1, ctypes.byref(n)) == ESTATE
        assert L.sift_mi_octave_dims(c._h, 0, ctypes.byref(a), ctypes.byref(b)) == ESTATE
        last = c._fetch(sum(len(r) for r in got))  # and the batch's result is still there
        assert np.array_equal(last[0], np.concatenate([r.keypoints_array for r in got]))
    finally:
        c.close()
    assert readbacks >= 5
    print(f"\nWALK profile {profile}: {len(WALK)} steps, {FRESH['contexts'] - fresh0} fresh contexts, "
          f"{readbacks} plane read-backs after a larger shape")
    assert FRESH["contexts"] - fresh0 <= 32


# ---------------------------------------------------------------------------
# (c) the graph cache under interleaving
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fetch", [True, False])
def test_graph_cache_under_interleaved_calls(pkg, fetch):
    """graph = 1, one context, default stream settings: A A A B A A C A A on
    device frames.  A is one 200 x 150 frame (captured at its second identical
    call, then replayed), B three frames of that size (the buffers were sized by a
    three-frame call made first, so B re-allocates nothing and the A after it
    finds its graph's key unchanged), C one 96 x 64 frame (a new plan: the
    allocation generation moves, A is seen anew and captured again).  Every
    result equals the graph = 0 result of the same call."""
    import torch
    frames = {"A": np.stack([_frame(200, 150, 0)]), "B": np.stack([_frame(200, 150, k) for k in (1, 2, 3)]),
              "C": np.stack([_frame(96, 64, 0)])}
    dev = {k: torch.from_numpy(v).cuda() for k, v in frames.items()}
    torch.cuda.synchronize()

    def run(c, k):
        t = dev[k]
        n, h, w = t.shape
        offs, res = c.sift_batch_device(t.data_ptr(), n, w, h, t.stride(1), t.stride(0), fetch=fetch)
        if fetch:
            return offs, res.keypoints_array, res.descriptors, res.keys
        kp_ptr, desc_ptr, m = c.device_results()
        assert m == int(offs[-1])
        return (offs,) + _copy_back(kp_ptr, desc_ptr, m)

    plain = _fresh(pkg)
    try:
        want = {k: run(plain, k) for k in "BAC"}
    finally:
        plain.close()
    assert all(int(want[k][0][-1]) > 0 for k in want)
    c = _fresh(pkg)
    try:
        c.set_path_option("graph", 1)
        replayed = []
        for step, k in enumerate("B" + "AAABAACAA"):
            before = c.stats()
            got = run(c, k)
            after = c.stats()
            for a, b in zip(got, want[k]):
                assert np.array_equal(a, b), (step, k)
            assert after["frames"] - before["frames"] == len(frames[k])
            # a replay enqueues no kernel from the host: the pyramid's launch count stands still
            if after["pyramid_launches"] == before["pyramid_launches"]:
                replayed.append(step)
    finally:
        c.close()
    # B A A A B A A C A A (steps 0..9).  The two A after the second B are
    # replays: B moved neither a buffer nor a high-water mark (the first B had
    # set them), so A's key still is the captured graph's.  The third A is one
    # too unless the first A raised a per-frame mark above the B frames'
    # average (the bounds are part of the key; then the capture happens one
    # call later).  After C the plan is new: A runs plainly, then is captured.
    print(f"\nGRAPH fetch {fetch}: replayed steps {replayed}")
    assert {5, 6} <= set(replayed) <= {3, 5, 6}, replayed
