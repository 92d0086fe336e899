"""Host-side mirror of the reference crate's public API over libsift_mi.so.

Reference: /root/reference/src/lib.rs (tnibler/sift-features @ 2024-10-22)

    pub fn sift(img: &GrayImage, features_limit: Option<usize>) -> SiftResult   (:71)
    pub fn sift_with_processing::<P: Processing>(img, features_limit)           (:76)
    pub trait Processing { gaussian_blur, resize_linear, resize_nearest }       (:86-90)
    pub struct SiftResult { keypoints: Vec<KeyPoint>, descriptors: Array2<u8> } (:41-46)
    pub struct KeyPoint { x, y, size, angle, response: f32 }                    (:50-56)
    #[doc(hidden)] precompute_images / sift_with_precomputed / compute_descriptor (:131, :147, :785)

Names, argument meaning and output layout follow the reference; the
computation is the HIP path (no CPU fallback).  Differences, all documented
in DESIGN.md:
  * `sift()` uses `ImageprocProcessing`, as the crate does (src/lib.rs:71-73);
    that profile restates imageproc 0.25 / image 0.25 arithmetic, which no
    reference test pins (parity unpinned).  `sift_with_processing(
    OpenCVProcessing, ...)` is the profile the reference's golden snapshots
    pin.
  * with a features_limit, ties in response keep emission order (the
    reference's `sort_unstable_by` leaves their order unspecified).
  * errors raise SiftMiError where the reference panics.
"""
import contextlib
import ctypes
import threading
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import SiftMiError, check, lib

PROFILE_OPENCV = 0
PROFILE_IMAGEPROC = 1
DESCRIPTOR_SIZE = 128


@dataclass
class KeyPoint:
    """src/lib.rs:50-56"""
    x: float
    y: float
    size: float
    angle: float
    response: float


class SiftResult:
    """src/lib.rs:41-46.  `keypoints_array` is the (n, 5) f32 table
    (x, y, size, angle, response); `descriptors` the (n, 128) u8 array whose
    row i belongs to keypoint i."""

    __slots__ = ("keypoints_array", "descriptors", "keys")

    def __init__(self, keypoints_array, descriptors, keys=None):
        self.keypoints_array = keypoints_array
        self.descriptors = descriptors
        self.keys = keys

    @property
    def keypoints(self):
        return [KeyPoint(*map(float, r)) for r in self.keypoints_array]

    def __len__(self):
        return len(self.keypoints_array)

    def __eq__(self, other):
        return (isinstance(other, SiftResult) and np.array_equal(self.keypoints_array, other.keypoints_array)
                and np.array_equal(self.descriptors, other.descriptors))

    def __repr__(self):
        return f"SiftResult(n={len(self)})"


class ResultBuffers:
    """Reusable host arrays for batch results (streaming callers: avoids a
    fresh allocation -- and its page faults -- per batch).  Grows on demand."""

    def __init__(self, capacity=0):
        self._alloc(capacity)

    def _alloc(self, n):
        self.kps = np.empty((n, 5), np.float32)
        self.desc = np.empty((n, DESCRIPTOR_SIZE), np.uint8)
        self.keys = np.empty(n, np.uint64)

    def views(self, n):
        if n > len(self.kps):
            self._alloc(max(n, 2 * len(self.kps)))
        return self.kps[:n], self.desc[:n], self.keys[:n]


def _u8_image(img):
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise TypeError("expected a 2-D uint8 GrayImage array (height, width)")
    if a.strides[1] != 1 or a.strides[0] < a.shape[1]:
        a = np.ascontiguousarray(a)
    return a


def _f32_image(img):
    a = np.ascontiguousarray(img, dtype=np.float32)
    if a.ndim != 2:
        raise TypeError("expected a 2-D f32 image (LumaFImage)")
    return a


class Tracks:
    """Feature tracks (Context.build_tracks_device; LABELLED EXTENSION).
    `track_of` (N,) int32: the track of each arena row from offsets[0] on, -1
    for none; `offsets` (len + 1,) uint32 into `obs`, a structured array of
    (seg, idx, x, y) with one record per member, a track's members by
    ascending row; `conflict` (len,) bool: the track holds two keypoints of
    one segment."""

    OBS = np.dtype([("seg", "<u4"), ("idx", "<u4"), ("x", "<f4"), ("y", "<f4")])
    __slots__ = ("track_of", "offsets", "obs", "conflict")

    def __init__(self, track_of, offsets, obs, conflict):
        self.track_of, self.offsets, self.obs, self.conflict = track_of, offsets, obs, conflict

    def __len__(self):
        return len(self.offsets) - 1

    def members(self, t):
        """The observations of track t."""
        if not 0 <= t < len(self):
            raise IndexError(t)
        return self.obs[self.offsets[t]:self.offsets[t + 1]]

    def __repr__(self):
        return f"Tracks(n={len(self)}, observations={len(self.obs)})"


class Selection:
    """Spread-limited keypoints (Context.select_spread_device; LABELLED
    EXTENSION).  `offsets` (n_segs + 1,) int64: the kept rows' segment bounds;
    `rows` (offsets[-1],) uint32: each kept row relative to its segment's first
    row, ascending within a segment (rows[offsets[s] + k] is what index k of
    segment s of the compact arena was in the original arena); `radius2` (N,)
    f32: the squared suppression radius of every input row (inf: nothing
    suppresses it), or None; `d_kps_ptr` / `d_desc_ptr`: the compact arena in
    device memory (kept keypoints and descriptors in the input's layout;
    d_desc_ptr is None when the call had no descriptors), valid until the
    context's next select call.  With `offsets` they go straight into
    match_pairs_device, verify_pairs_device and the other arena calls."""

    __slots__ = ("offsets", "rows", "radius2", "d_kps_ptr", "d_desc_ptr")

    def __init__(self, offsets, rows, radius2, d_kps_ptr, d_desc_ptr):
        self.offsets, self.rows, self.radius2 = offsets, rows, radius2
        self.d_kps_ptr, self.d_desc_ptr = d_kps_ptr, d_desc_ptr

    def __len__(self):
        return len(self.rows)

    def segment_rows(self, s):
        """The kept rows of segment s (relative to its first row)."""
        return self.rows[self.offsets[s]:self.offsets[s + 1]]

    def __repr__(self):
        return f"Selection(segments={len(self.offsets) - 1}, kept={len(self.rows)})"


def _match_arrays(a, lo, hi):
    """Rows lo..hi of a sift_mi_match record array as (query_idx, train_idx, distance)."""
    a = a[lo:hi]
    return (a["query_idx"].astype(np.int32), a["train_idx"].astype(np.int32), a["distance"].astype(np.float32))


def _limit(features_limit):
    if features_limit is None:
        return -1
    if features_limit < 0:
        raise ValueError("features_limit must be >= 0 or None")
    return int(features_limit)


class Context:
    """One device context (libsift_mi `sift_mi_ctx`): one HIP stream, pooled
    device buffers.  Not thread-safe; use one per thread / GPU."""

    def __init__(self, device=0, processing=None):
        processing = processing or OpenCVProcessing
        self.profile = processing.profile
        self.device = device
        h = ctypes.c_void_p()
        check(lib().sift_mi_create(device, self.profile, ctypes.byref(h)))
        self._h = h
        self._generation = 0
        self._keep_dev = False  # sift_mi_set_keep_on_device state
        self._path_values = {}  # sift_mi_set_path_option values set through this object

    def close(self):
        if getattr(self, "_h", None):
            lib().sift_mi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration ----------------------------------------------------
    def set_stream(self, hip_stream_handle):
        """Run later calls on the caller's hipStream_t (sift_mi_set_stream),
        e.g. `torch.cuda.Stream().cuda_stream`: every kernel and copy of a
        call is ordered after the work already enqueued on that stream, so
        inputs produced there need no host synchronisation, and every call
        returns after its results are complete.  Close the context, or
        set_stream(None), before the stream is destroyed.

        None or 0 restores the context's own non-blocking stream, which does
        NOT synchronise with the legacy default stream.  torch's default
        stream is that stream: `torch.cuda.current_stream().cuda_stream` is 0
        there (observed on the MI355X with torch 2.10 / ROCm 7.0), so passing
        it selects the context's own stream and orders nothing.  A caller on
        torch's default stream must synchronise before the call
        (`torch.cuda.current_stream().synchronize()`), or do its work on a
        side stream and pass that."""
        check(lib().sift_mi_set_stream(self._h, ctypes.c_void_p(hip_stream_handle or 0)))

    def set_exact_descriptors(self, exact=True):
        """Bit-exact descriptor accumulation order (slower); default off."""
        check(lib().sift_mi_set_exact_descriptors(self._h, 1 if exact else 0))

    def set_max_octaves(self, max_octaves):
        """LABELLED EXTENSION (not in the crate): cap the octave count (0 = the
        crate's formula, src/lib.rs:133-134).  The result is the uncapped
        result's keypoints of octaves < max_octaves."""
        check(lib().sift_mi_set_max_octaves(self._h, int(max_octaves)))

    def set_sample_counting(self, on=True):
        """Measurement only: count the gradient samples the orientation and
        descriptor kernels evaluate (stats() orient_samples / desc_samples)."""
        check(lib().sift_mi_set_sample_counting(self._h, 1 if on else 0))

    def set_row_band(self, band, n_bands):
        """Keypoint stages over octave rows [H_o*band/n_bands, H_o*(band+1)/n_bands)
        only (include/sift_mi.h); band 0 of 1 = the whole frame.  Merge the
        bands' results with shard.merge_bands."""
        check(lib().sift_mi_set_row_band(self._h, int(band), int(n_bands)))

    def set_chunk(self, images_per_chunk):
        check(lib().sift_mi_set_chunk(self._h, int(images_per_chunk)))

    def stats(self):
        s = _lib.Stats()
        check(lib().sift_mi_get_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def reset_stats(self):
        check(lib().sift_mi_reset_stats(self._h))

    # -- results ------------------------------------------------------------
    def _keep(self, on):
        """Results to host buffers (False: every host-returning call) or left
        in HBM (True: sift_batch_device(..., fetch=False))."""
        if bool(on) != self._keep_dev:
            check(lib().sift_mi_set_keep_on_device(self._h, 1 if on else 0))
            self._keep_dev = bool(on)

    def _fetch(self, n, with_keys=True, out=None):
        if out is not None:
            kps, desc, keys = out.views(n)
        else:
            kps = np.empty((n, 5), np.float32)
            desc = np.empty((n, DESCRIPTOR_SIZE), np.uint8)
            keys = np.empty(n, np.uint64) if with_keys else None
        check(lib().sift_mi_fetch(self._h, kps.ctypes.data, desc.ctypes.data, n))
        if with_keys:
            check(lib().sift_mi_fetch_keys(self._h, keys.ctypes.data, n))
        else:
            keys = None
        return kps, desc, keys

    # -- sift (src/lib.rs:71-81) ---------------------------------------------
    def sift(self, img, features_limit=None):
        a = _u8_image(img)
        n = ctypes.c_size_t()
        self._keep(False)
        check(lib().sift_mi_extract(self._h, a.ctypes.data, a.shape[1], a.shape[0], a.strides[0],
                                    _limit(features_limit), ctypes.byref(n)))
        return SiftResult(*self._fetch(n.value))

    def sift_batch(self, frames, features_limit=None):
        """One `sift()` per frame of an (n, h, w) u8 array; returns a list."""
        f = np.ascontiguousarray(frames, dtype=np.uint8)
        if f.ndim != 3:
            raise TypeError("expected (n, height, width) uint8 frames")
        n, h, w = f.shape
        ptrs = (ctypes.c_void_p * n)(*[f[i].ctypes.data for i in range(n)])
        offs = (ctypes.c_size_t * (n + 1))()
        self._keep(False)
        check(lib().sift_mi_extract_batch(self._h, ptrs, n, w, h, w, _limit(features_limit), offs))
        kps, desc, keys = self._fetch(offs[n])
        return [SiftResult(kps[offs[i]:offs[i + 1]], desc[offs[i]:offs[i + 1]], keys[offs[i]:offs[i + 1]])
                for i in range(n)]

    def sift_batch_device(self, d_frames_ptr, n, width, height, row_stride, frame_pitch,
                          features_limit=None, fetch=True, out=None):
        """Device-resident frames (e.g. a torch.uint8 cuda tensor's data_ptr()).
        Returns per-frame offsets and, with fetch, the concatenated results.
        `out` (a ResultBuffers) receives the results in reused host arrays;
        the returned SiftResult then holds views into it, valid until the
        buffers are reused."""
        offs = (ctypes.c_size_t * (n + 1))()
        self._keep(not fetch)
        check(lib().sift_mi_extract_batch_device(self._h, ctypes.c_void_p(d_frames_ptr), frame_pitch, n, width,
                                                 height, row_stride, _limit(features_limit), offs))
        offsets = np.array(offs[:], dtype=np.int64)
        if not fetch:
            return offsets, None
        return offsets, SiftResult(*self._fetch(int(offsets[-1]), out=out))

    def set_pipeline_lanes(self, lanes):
        """2 (default): consecutive batch chunks overlap on two streams; 1: serial."""
        check(lib().sift_mi_set_pipeline_lanes(self._h, int(lanes)))

    def device_results(self):
        """(keypoints device pointer, descriptors device pointer, n) of the last
        sift_batch_device(..., fetch=False): every frame's results, concatenated
        in frame order, in HBM.  Valid until the next extraction call; the
        match calls only read them."""
        kp, desc, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        check(lib().sift_mi_device_results(self._h, ctypes.byref(kp), ctypes.byref(desc), ctypes.byref(n)))
        return kp.value, desc.value, n.value

    def read_batch_scale_space(self, frame, octave, dims=None):
        """(6, h, w) f32 Gaussians of `octave` of `frame` of the last call, as
        its pyramid left them (valid when that call ran as one chunk; a
        validation read-back, sift_mi_read_batch_scale_space).  The octave's
        (w, h) come from the library (sift_mi_batch_octave_dims); `dims`, if
        given, must equal them."""
        w, h = ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().sift_mi_batch_octave_dims(self._h, int(octave), ctypes.byref(w), ctypes.byref(h)))
        if dims is not None and tuple(dims) != (w.value, h.value):
            raise ValueError(f"dims {tuple(dims)} != the batch octave's {(w.value, h.value)}")
        out = np.empty((6, h.value, w.value), np.float32)
        check(lib().sift_mi_read_batch_scale_space(self._h, int(frame), int(octave), out.ctypes.data, out.size))
        return out

    # kernel-path switches (include/sift_mi.h sift_mi_path_option): test /
    # diagnostic only; the defaults are the product path
    PATH_OPTIONS = {"tile_blur": (0, 0), "pair_blur": (1, 1), "seed_pair": (2, 1), "tail": (3, 1),
                    "fused_detect": (4, 1), "early": (5, 1), "desc_first": (6, 1), "graph": (7, 0),
                    "band_drift": (8, 24), "bound_shrink": (9, 1),
                    "large_first": (11, 1),
                    "onesweep": (12, 0), "bd_pair": (13, 1), "bd_waves": (14, 8192),
                    "chunk_mode": (15, 1), "guided_cull": (16, 1)}

    def set_path_option(self, name, value):
        """One kernel-path switch (sift_mi_set_path_option), e.g.
        set_path_option("pair_blur", 0)."""
        check(lib().sift_mi_set_path_option(self._h, self.PATH_OPTIONS[name][0], int(value)))
        self._path_values[name] = int(value)

    def path_option(self, name):
        """The switch's current value (as last set through this object, else
        its default)."""
        return self._path_values.get(name, self.PATH_OPTIONS[name][1])

    @contextlib.contextmanager
    def path_options(self, **opts):
        """Kernel-path switches for the duration of a with-block, then the
        values they had before it."""
        before = {k: self.path_option(k) for k in opts}
        try:
            for k, v in opts.items():
                self.set_path_option(k, v)
            yield self
        finally:
            for k, v in before.items():
                self.set_path_option(k, v)

    # -- precompute_images / sift_with_precomputed (src/lib.rs:123-177) ------
    def precompute_images(self, img):
        a = _u8_image(img)
        n = ctypes.c_size_t()
        check(lib().sift_mi_precompute(self._h, a.ctypes.data, a.shape[1], a.shape[0], a.strides[0],
                                       ctypes.byref(n)))
        self._generation += 1
        return PrecomputedImages(self, n.value, self._generation)

    def sift_with_precomputed(self, pre, features_limit=None):
        pre._check()
        n = ctypes.c_size_t()
        self._keep(False)
        check(lib().sift_mi_sift_with_precomputed(self._h, _limit(features_limit), ctypes.byref(n)))
        return SiftResult(*self._fetch(n.value))

    # -- compute_descriptor (src/lib.rs:785) -----------------------------------
    def compute_descriptor(self, img, x, y, scale, orientation):
        a = _f32_image(img)
        out = np.zeros(DESCRIPTOR_SIZE, np.uint8)
        check(lib().sift_mi_compute_descriptor(self._h, a.ctypes.data, a.shape[1], a.shape[0], float(x),
                                               float(y), float(scale), float(orientation), out.ctypes.data))
        return out

    # -- matching (examples/sift-match.rs:30-35) -----------------------------
    def match_descriptors(self, query, train, cross_check=True, ratio=None):
        """cv::BFMatcher(NORM_L2, crossCheck).match(query, train) on the GPU.
        query / train: (n, 128) u8 descriptors.  Returns (query_idx, train_idx,
        distance) arrays in query order.  LABELLED EXTENSION: with `ratio`
        (0 < ratio <= 1) a query is kept only if its nearest distance is below
        ratio * its second nearest (Lowe's ratio test; sift_mi_match_ratio)."""
        q = np.ascontiguousarray(query, dtype=np.uint8).reshape(-1, DESCRIPTOR_SIZE)
        t = np.ascontiguousarray(train, dtype=np.uint8).reshape(-1, DESCRIPTOR_SIZE)
        out = (_lib.Match * max(len(q), 1))()
        n = ctypes.c_size_t()
        if ratio is None:
            check(lib().sift_mi_match_descriptors(self._h, q.ctypes.data, len(q), t.ctypes.data, len(t),
                                                  1 if cross_check else 0, out, len(q), ctypes.byref(n)))
        else:
            check(lib().sift_mi_match_ratio(self._h, q.ctypes.data, len(q), t.ctypes.data, len(t), float(ratio),
                                            1 if cross_check else 0, out, len(q), ctypes.byref(n)))
        return _match_arrays(np.ctypeslib.as_array(out), 0, n.value)

    def match_neighbors(self, query, train):
        """LABELLED EXTENSION: cv::BFMatcher(NORM_L2).knnMatch(query, train, 2).
        Returns (idx (n, 2) int32, dist (n, 2) f32): each query's two nearest
        train rows by (distance, index); -1 / inf where train has fewer rows."""
        q = np.ascontiguousarray(query, dtype=np.uint8).reshape(-1, DESCRIPTOR_SIZE)
        t = np.ascontiguousarray(train, dtype=np.uint8).reshape(-1, DESCRIPTOR_SIZE)
        out = (_lib.Neighbors * max(len(q), 1))()
        check(lib().sift_mi_match_neighbors(self._h, q.ctypes.data, len(q), t.ctypes.data, len(t), out))
        a = np.ctypeslib.as_array(out)[: len(q)]
        return a["train_idx"].astype(np.int32).reshape(-1, 2), a["distance"].astype(np.float32).reshape(-1, 2)

    def match_pairs_device(self, d_desc_ptr, offsets, pairs, ratio=None, cross_check=True):
        """Match (query segment, train segment) pairs of device-resident
        descriptors in one launch sequence (sift_mi_match_pairs_device).
        d_desc_ptr: device pointer of (n, 128) u8 rows; segment s is rows
        offsets[s]..offsets[s+1]; pairs: (query_seg, train_seg) tuples.
        Returns one (query_idx, train_idx, distance) triple per pair, indices
        relative to the pair's segments."""
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        if offs.ndim != 1 or len(offs) < 1 or (offs < 0).any():
            raise ValueError("offsets: n_segs + 1 non-negative row numbers")
        c_offs = (ctypes.c_size_t * len(offs))(*[int(v) for v in offs])
        pr = [(int(a), int(b)) for a, b in pairs]
        c_pairs = (_lib.SegPair * max(len(pr), 1))(*[_lib.SegPair(a, b) for a, b in pr])
        n_seg = len(offs) - 1
        cap = sum(int(offs[a + 1] - offs[a]) for a, _ in pr if 0 <= a < n_seg and offs[a + 1] >= offs[a])
        out = (_lib.Match * max(cap, 1))()
        po = (ctypes.c_size_t * (len(pr) + 1))()
        check(lib().sift_mi_match_pairs_device(self._h, ctypes.c_void_p(d_desc_ptr), c_offs, n_seg, c_pairs, len(pr),
                                               float(ratio or 0.0), 1 if cross_check else 0, out, cap, po))
        a = np.ctypeslib.as_array(out)
        return [_match_arrays(a, po[p], po[p + 1]) for p in range(len(pr))]

    def match_frames(self, offsets, pairs, ratio=None, cross_check=True):
        """match_pairs_device on the descriptors the last
        sift_batch_device(..., fetch=False) left in HBM: `offsets` as that
        call returned them, `pairs` of (query frame, train frame)."""
        _, d_desc, n = self.device_results()
        if int(offsets[-1]) > n:
            raise ValueError("offsets reach beyond the device results")
        return self.match_pairs_device(d_desc, offsets, pairs, ratio, cross_check)

    # -- geometric verification (LABELLED EXTENSION: not in the crate) --------
    @staticmethod
    def _ransac(threshold, iterations, seed, refit_rounds):
        return _lib.RansacParams(float(threshold), int(iterations), int(seed) & 0xFFFFFFFF, int(refit_rounds))

    @staticmethod
    def _match_records(matches):
        """(query_idx, train_idx, distance) triples -> one sift_mi_match array and the triples' offsets."""
        po = np.zeros(len(matches) + 1, np.int64)
        po[1:] = np.cumsum([len(m[0]) for m in matches])
        rec = np.zeros(max(int(po[-1]), 1), np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("distance", "<f4")]))
        for p, m in enumerate(matches):
            r = rec[po[p]:po[p + 1]]
            r["query_idx"], r["train_idx"] = m[0], m[1]
            if len(m) > 2:
                r["distance"] = m[2]
        return rec, po

    @staticmethod
    def _verify_result(model, mask):
        info = {"n_matches": model.n_matches, "n_inliers": model.n_inliers,
                "best_hypothesis": model.best_hypothesis, "refits": model.refits}
        values = model.f if isinstance(model, _lib.Fundamental) else model.h
        return np.array(values[:], np.float32).reshape(3, 3), mask.astype(bool), info

    @staticmethod
    def _verify_model(model, sampling="uniform"):
        """The record type and the two entry points of `model` under `sampling`."""
        if sampling not in ("uniform", "progressive"):
            raise ValueError(f"sampling must be 'uniform' or 'progressive', not {sampling!r}")
        prog = sampling == "progressive"
        if model == "homography":
            if prog:
                return (_lib.Homography, lib().sift_mi_verify_pairs_progressive_device,
                        lib().sift_mi_verify_matches_progressive)
            return _lib.Homography, lib().sift_mi_verify_pairs_device, lib().sift_mi_verify_matches
        if model == "fundamental":
            if prog:
                return (_lib.Fundamental, lib().sift_mi_verify_pairs_epipolar_progressive_device,
                        lib().sift_mi_verify_matches_epipolar_progressive)
            return _lib.Fundamental, lib().sift_mi_verify_pairs_epipolar_device, lib().sift_mi_verify_matches_epipolar
        raise ValueError(f"model must be 'homography' or 'fundamental', not {model!r}")

    @staticmethod
    def _quality_args(sampling, quality, po):
        """The extra arguments of a progressive call: (the f32 array to keep
        alive, [its pointer]); nothing for a uniform one.  `quality`: one array
        per pair (or None for all: the matches' distance)."""
        if sampling != "progressive":
            if quality is not None:
                raise ValueError("quality is only read with sampling='progressive'")
            return None, []
        if quality is None:
            return None, [None]
        if len(quality) != len(po) - 1:
            raise ValueError("one quality array per pair")
        q = np.zeros(max(int(po[-1]), 1), np.float32)
        for p, v in enumerate(quality):
            v = np.asarray(v, np.float32).reshape(-1)
            if len(v) != po[p + 1] - po[p]:
                raise ValueError("one quality per match")
            q[po[p]:po[p + 1]] = v
        return q, [q.ctypes.data]

    def verify_pairs_device(self, d_kps_ptr, offsets, pairs, matches, threshold=3.0, iterations=1024, seed=0,
                            refit_rounds=2, model="homography", sampling="uniform", quality=None):
        """LABELLED EXTENSION (the crate has nothing like it): per pair a RANSAC
        homography on its matches with up to `refit_rounds` least-squares
        refits on the inliers (sift_mi_verify_pairs_device; the rules are
        tests/verify_ref.py's).  d_kps_ptr: device pointer of the keypoints
        (device_results()[0]); offsets / pairs as for match_pairs_device;
        matches: the (query_idx, train_idx, distance) triples it returned, one
        per pair (possibly filtered).  Returns per pair (H (3, 3) f32 mapping
        the query keypoint's (x, y, 1) to the train image, inlier mask bool,
        info dict: n_matches, n_inliers, best_hypothesis, refits); H is all
        zero and best_hypothesis -1 where the pair has no model.

        model="fundamental" (another labelled extension, for a moving camera
        in a 3-D scene) fits a RANSAC fundamental matrix instead
        (sift_mi_verify_pairs_epipolar_device; tests/epipolar_ref.py): 8-point
        samples, `threshold` is the Sampson distance in px, and the first
        item is F (3, 3) f32 with (X, Y, 1) F (x, y, 1)^T = 0 for a query
        keypoint (x, y) and its train keypoint (X, Y), largest entry 1.  F is
        rank 2 (up to f32 rounding) iff info["refits"] >= 1, the raw 8-point
        solution otherwise; a pair needs 8 matches.  A planar scene satisfies
        a family of F (use the homography there), and under uniform sampling
        1024 hypotheses suit inlier shares >= 0.5.  Any other `model` raises
        ValueError.

        sampling="progressive" (a further labelled extension; PROSAC, the rule
        is tests/prosac_ref.py's) ranks each pair's matches by `quality`, one
        array per pair, lower is better, finite with the sign bit clear (None:
        the matches' distance), and hypothesis h draws from the best n_h of
        them, n_h growing with h (sift_mi_verify_pairs_progressive_device /
        ..._epipolar_progressive_device); it reaches lower inlier shares with
        the same `iterations`.  The masks stay in the matches' order.
        sampling="uniform" is the call and the result of before."""
        record, call, _ = self._verify_model(model, sampling)
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        if offs.ndim != 1 or len(offs) < 1 or (offs < 0).any():
            raise ValueError("offsets: n_segs + 1 non-negative row numbers")
        pr = [(int(a), int(b)) for a, b in pairs]
        if len(matches) != len(pr):
            raise ValueError("one (query_idx, train_idx, distance) triple per pair")
        rec, po = self._match_records(matches)
        c_offs = (ctypes.c_size_t * len(offs))(*[int(v) for v in offs])
        c_po = (ctypes.c_size_t * len(po))(*[int(v) for v in po])
        c_pairs = (_lib.SegPair * max(len(pr), 1))(*[_lib.SegPair(a, b) for a, b in pr])
        models = (record * max(len(pr), 1))()
        mask = np.zeros(max(int(po[-1]), 1), np.uint8)
        prm = self._ransac(threshold, iterations, seed, refit_rounds)
        _q, extra = self._quality_args(sampling, quality, po)
        check(call(self._h, ctypes.c_void_p(d_kps_ptr), c_offs, len(offs) - 1, c_pairs, len(pr), rec.ctypes.data, c_po,
                   *extra, ctypes.byref(prm), models, mask.ctypes.data))
        return [self._verify_result(models[p], mask[po[p]:po[p + 1]]) for p in range(len(pr))]

    def verify_frames(self, offsets, pairs, matches, threshold=3.0, iterations=1024, seed=0, refit_rounds=2,
                      model="homography", sampling="uniform", quality=None):
        """verify_pairs_device on the keypoints the last
        sift_batch_device(..., fetch=False) left in HBM, e.g. on what
        match_frames(offsets, pairs, ...) returned."""
        self._verify_model(model, sampling)
        d_kps, _, n = self.device_results()
        if int(offsets[-1]) > n:
            raise ValueError("offsets reach beyond the device results")
        return self.verify_pairs_device(d_kps, offsets, pairs, matches, threshold, iterations, seed, refit_rounds,
                                        model=model, sampling=sampling, quality=quality)

    def verify_matches(self, kps_q, kps_t, matches, threshold=3.0, iterations=1024, seed=0, refit_rounds=2,
                       model="homography", sampling="uniform", quality=None):
        """The one-pair form on host keypoints (sift_mi_verify_matches): kps_q /
        kps_t are (n, 5) f32 keypoint arrays (SiftResult.keypoints_array; only
        x, y are read), matches one (query_idx, train_idx, distance) triple.
        Returns (H, inlier mask, info) as verify_pairs_device does per pair,
        (F, inlier mask, info) with model="fundamental"
        (sift_mi_verify_matches_epipolar).  sampling="progressive": as
        verify_pairs_device, `quality` one array over the matches or None."""
        record, _, call = self._verify_model(model, sampling)
        q = np.ascontiguousarray(kps_q, dtype=np.float32).reshape(-1, 5)
        t = np.ascontiguousarray(kps_t, dtype=np.float32).reshape(-1, 5)
        rec, po = self._match_records([matches])
        out = record()
        mask = np.zeros(max(int(po[-1]), 1), np.uint8)
        prm = self._ransac(threshold, iterations, seed, refit_rounds)
        _q, extra = self._quality_args(sampling, None if quality is None else [quality], po)
        check(call(self._h, q.ctypes.data, len(q), t.ctypes.data, len(t), rec.ctypes.data, int(po[-1]),
                   *extra, ctypes.byref(prm), ctypes.byref(out), mask.ctypes.data))
        return self._verify_result(out, mask[:po[-1]])

    # -- guided matching (LABELLED EXTENSION: not in the crate) ----------------
    @staticmethod
    def _guided(threshold, ratio, max_distance, cross_check, model):
        if model not in _lib.MODEL_KINDS:
            raise ValueError(f"model must be 'homography' or 'fundamental', not {model!r}")
        return _lib.MODEL_KINDS[model], _lib.GuidedParams(float(threshold), float(ratio or 0.0),
                                                          float(max_distance or 0.0), 1 if cross_check else 0)

    @staticmethod
    def _model_array(models):
        """(H, mask, info) tuples of verify_frames or bare 3 x 3 arrays -> (n, 9) f32."""
        rows = [np.asarray(m[0] if isinstance(m, tuple) else m, np.float32).reshape(9) for m in models]
        return np.ascontiguousarray(np.stack(rows) if rows else np.zeros((0, 9), np.float32))

    def match_pairs_guided_device(self, d_desc_ptr, d_kps_ptr, offsets, pairs, models, threshold=3.0,
                                  model="homography", ratio=None, max_distance=None, cross_check=True):
        """LABELLED EXTENSION: match_pairs_device again, a query keypoint
        competing only for the train keypoints its pair's model admits
        (sift_mi_match_pairs_guided_device; the rule is tests/guided_ref.py's).
        d_kps_ptr: device pointer of the keypoints of the same rows;
        models: per pair the (H, mask, info) tuple of verify_pairs_device or a
        bare 3 x 3 array (H, or F with model="fundamental"); `threshold` as
        the verification read it.  Admissible = the verification's own inlier
        test on (query keypoint, train keypoint).  Nearest, second nearest
        and the cross check run over the admissible candidates only; with
        `ratio` a query with a single admissible candidate PASSES (its second
        distance is +inf; the unguided ratio test rejects it), and
        `max_distance` keeps a query only if its distance is <= it.  A pair
        with an all-zero model (no model) gets no matches.  Returns one
        (query_idx, train_idx, distance) triple per pair."""
        kind, prm = self._guided(threshold, ratio, max_distance, cross_check, model)
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        if offs.ndim != 1 or len(offs) < 1 or (offs < 0).any():
            raise ValueError("offsets: n_segs + 1 non-negative row numbers")
        pr = [(int(a), int(b)) for a, b in pairs]
        g = self._model_array(models)
        if len(g) != len(pr):
            raise ValueError("one model per pair")
        c_offs = (ctypes.c_size_t * len(offs))(*[int(v) for v in offs])
        c_pairs = (_lib.SegPair * max(len(pr), 1))(*[_lib.SegPair(a, b) for a, b in pr])
        n_seg = len(offs) - 1
        cap = sum(int(offs[a + 1] - offs[a]) for a, _ in pr if 0 <= a < n_seg and offs[a + 1] >= offs[a])
        out = (_lib.Match * max(cap, 1))()
        po = (ctypes.c_size_t * (len(pr) + 1))()
        g = g if len(g) else np.zeros((1, 9), np.float32)
        check(lib().sift_mi_match_pairs_guided_device(self._h, ctypes.c_void_p(d_desc_ptr), ctypes.c_void_p(d_kps_ptr),
                                                      c_offs, n_seg, c_pairs, len(pr), kind, g.ctypes.data,
                                                      ctypes.byref(prm), out, cap, po))
        a = np.ctypeslib.as_array(out)
        return [_match_arrays(a, po[p], po[p + 1]) for p in range(len(pr))]

    def match_frames_guided(self, offsets, pairs, models, threshold=3.0, model="homography", ratio=None,
                            max_distance=None, cross_check=True):
        """match_pairs_guided_device on the keypoints and descriptors the last
        sift_batch_device(..., fetch=False) left in HBM, e.g. with what
        verify_frames(offsets, pairs, ...) returned as `models`."""
        d_kps, d_desc, n = self.device_results()
        if int(offsets[-1]) > n:
            raise ValueError("offsets reach beyond the device results")
        return self.match_pairs_guided_device(d_desc, d_kps, offsets, pairs, models, threshold, model, ratio,
                                              max_distance, cross_check)

    def match_guided(self, desc_q, kps_q, desc_t, kps_t, model_matrix, threshold=3.0, model="homography", ratio=None,
                     max_distance=None, cross_check=True):
        """The one-pair form on host arrays (sift_mi_match_guided): (n, 128) u8
        descriptors and (n, 5) f32 keypoint arrays of the query and the train
        image, one 3 x 3 model (or a verify_matches tuple).  Returns
        (query_idx, train_idx, distance)."""
        kind, prm = self._guided(threshold, ratio, max_distance, cross_check, model)
        q = np.ascontiguousarray(desc_q, dtype=np.uint8).reshape(-1, DESCRIPTOR_SIZE)
        t = np.ascontiguousarray(desc_t, dtype=np.uint8).reshape(-1, DESCRIPTOR_SIZE)
        kq = np.ascontiguousarray(kps_q, dtype=np.float32).reshape(-1, 5)
        kt = np.ascontiguousarray(kps_t, dtype=np.float32).reshape(-1, 5)
        if len(kq) != len(q) or len(kt) != len(t):
            raise ValueError("one keypoint row per descriptor row")
        g = self._model_array([model_matrix])
        out = (_lib.Match * max(len(q), 1))()
        n = ctypes.c_size_t()
        check(lib().sift_mi_match_guided(self._h, q.ctypes.data, kq.ctypes.data, len(q), t.ctypes.data, kt.ctypes.data,
                                         len(t), kind, g.ctypes.data, ctypes.byref(prm), out, len(q), ctypes.byref(n)))
        return _match_arrays(np.ctypeslib.as_array(out), 0, n.value)

    def guided_counters(self):
        """{"tiles", "culled_waves"} of the guided calls since the last
        reset_stats(): the 128 x 128 tiles they covered and the waves (four
        per tile) that skipped their block because the model admits none of
        it (sift_mi_guided_counters; path option "guided_cull")."""
        tiles, culled = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().sift_mi_guided_counters(self._h, ctypes.byref(tiles), ctypes.byref(culled)))
        return {"tiles": tiles.value, "culled_waves": culled.value}

    # -- feature tracks (LABELLED EXTENSION: not in the crate) -------------------
    def build_tracks_device(self, d_kps_ptr, offsets, pairs, matches, keep=None, min_length=2, conflicts="flag"):
        """LABELLED EXTENSION: link the pairs' matches across the segments
        into tracks on the device (sift_mi_build_tracks_device; the rule is
        tests/tracks_ref.py's).  A track is a connected component of the graph
        whose nodes are the arena rows and whose edges are the kept matches,
        with at least `min_length` (>= 2) rows.  d_kps_ptr, offsets, pairs,
        matches as for verify_pairs_device; `keep`: per pair a boolean mask
        over its matches, or the (model, mask, info) tuple verify_pairs_device
        returned for it (None: every match).  A track with two keypoints of
        one segment is in conflict: conflicts="flag" keeps it and marks it in
        Tracks.conflict, conflicts="drop" leaves it out.  Tracks are numbered
        by their smallest row.  Returns a Tracks."""
        if conflicts not in ("flag", "drop"):
            raise ValueError(f"conflicts must be 'flag' or 'drop', not {conflicts!r}")
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        if offs.ndim != 1 or len(offs) < 1 or (offs < 0).any():
            raise ValueError("offsets: n_segs + 1 non-negative row numbers")
        pr = [(int(a), int(b)) for a, b in pairs]
        if len(matches) != len(pr):
            raise ValueError("one (query_idx, train_idx, distance) triple per pair")
        rec, po = self._match_records(matches)
        mask = None
        if keep is not None:
            if len(keep) != len(pr):
                raise ValueError("one keep mask per pair")
            mask = np.zeros(max(int(po[-1]), 1), np.uint8)
            for p, k in enumerate(keep):
                k = np.asarray(k[1] if isinstance(k, tuple) else k).astype(bool).reshape(-1)
                if len(k) != po[p + 1] - po[p]:
                    raise ValueError(f"keep mask of pair {p}: one entry per match")
                mask[po[p]:po[p + 1]] = k
        n = max(int(offs[-1] - offs[0]), 0)
        c_offs = (ctypes.c_size_t * len(offs))(*[int(v) for v in offs])
        c_po = (ctypes.c_size_t * len(po))(*[int(v) for v in po])
        c_pairs = (_lib.SegPair * max(len(pr), 1))(*[_lib.SegPair(a, b) for a, b in pr])
        track_of = np.empty(max(n, 1), np.int32)
        t_offs = np.zeros(n // 2 + 2, np.uint32)
        obs = np.zeros(max(n, 1), Tracks.OBS)
        conflict = np.zeros(n // 2 + 1, np.uint8)
        n_tracks = ctypes.c_uint32()
        prm = _lib.TrackParams(int(min_length), 1 if conflicts == "drop" else 0)
        check(lib().sift_mi_build_tracks_device(self._h, ctypes.c_void_p(d_kps_ptr), c_offs, len(offs) - 1, c_pairs,
                                                len(pr), rec.ctypes.data, c_po,
                                                None if mask is None else mask.ctypes.data, ctypes.byref(prm),
                                                track_of.ctypes.data, ctypes.byref(n_tracks), t_offs.ctypes.data,
                                                obs.ctypes.data, conflict.ctypes.data))
        nt = n_tracks.value
        t_offs = t_offs[:nt + 1].copy()
        return Tracks(track_of[:n], t_offs, obs[:int(t_offs[-1])].copy(), conflict[:nt].astype(bool))

    def track_frames(self, offsets, pairs, matches, keep=None, min_length=2, conflicts="flag"):
        """build_tracks_device on the keypoints the last
        sift_batch_device(..., fetch=False) left in HBM, e.g. on what
        match_frames returned as `matches` and verify_frames as `keep`."""
        if conflicts not in ("flag", "drop"):
            raise ValueError(f"conflicts must be 'flag' or 'drop', not {conflicts!r}")
        d_kps, _, n = self.device_results()
        if int(offsets[-1]) > n:
            raise ValueError("offsets reach beyond the device results")
        return self.build_tracks_device(d_kps, offsets, pairs, matches, keep, min_length, conflicts)

    def track_counters(self):
        """{"kernel_ms", "edges"} of the track calls since the last
        reset_stats(): the time between two events around their launch
        sequences and the kept matches they linked (sift_mi_track_counters)."""
        ms, edges = ctypes.c_double(), ctypes.c_uint64()
        check(lib().sift_mi_track_counters(self._h, ctypes.byref(ms), ctypes.byref(edges)))
        return {"kernel_ms": ms.value, "edges": edges.value}

    # -- frame-pair proposal (LABELLED EXTENSION: not in the crate) ----------------
    def propose_pairs_device(self, d_desc_ptr, d_kps_ptr, offsets, subset=128, ratio=0.8, min_matches=8,
                             max_partners=0):
        """LABELLED EXTENSION: which segments of an unordered arena to match,
        by preemptive matching on the device (sift_mi_propose_pairs_device;
        the rule is tests/pairs_ref.py's).  The `subset` (1..128) rows with
        the largest keypoint size of every segment are matched between all
        segment pairs (cross check, ratio test unless ratio is 0 / None);
        scores[a, b] counts the matches kept from a to b.  A pair a < b with
        max(scores[a, b], scores[b, a]) >= min_matches is a candidate; with
        max_partners > 0 each segment keeps its max_partners best candidates
        and a pair is proposed when either side keeps it.  Returns (pairs,
        scores): the proposed (a, b) sorted, ready for match_pairs_device, and
        the (n, n) uint32 score matrix.  The default min_matches suits the
        synthetic content it was set on, not every input."""
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        if offs.ndim != 1 or len(offs) < 1 or (offs < 0).any():
            raise ValueError("offsets: n_segs + 1 non-negative row numbers")
        n = len(offs) - 1
        c_offs = (ctypes.c_size_t * len(offs))(*[int(v) for v in offs])
        prm = _lib.PairParams(int(subset), float(ratio or 0.0), int(min_matches), int(max_partners))
        scores = np.zeros((n, n), np.uint32)
        cap = n * (n - 1) // 2
        out = (_lib.SegPair * max(cap, 1))()
        k = ctypes.c_size_t()
        check(lib().sift_mi_propose_pairs_device(self._h, ctypes.c_void_p(d_desc_ptr), ctypes.c_void_p(d_kps_ptr),
                                                 c_offs, n, ctypes.byref(prm), scores.ctypes.data if n else None, out,
                                                 cap, ctypes.byref(k)))
        return [(out[i].query_seg, out[i].train_seg) for i in range(k.value)], scores

    def propose_frames(self, offsets, subset=128, ratio=0.8, min_matches=8, max_partners=0):
        """propose_pairs_device on the results the last
        sift_batch_device(..., fetch=False) left in HBM; the pairs go to
        match_frames as they are."""
        d_kps, d_desc, n = self.device_results()
        if int(offsets[-1]) > n:
            raise ValueError("offsets reach beyond the device results")
        return self.propose_pairs_device(d_desc, d_kps, offsets, subset, ratio, min_matches, max_partners)

    def pair_counters(self):
        """{"kernel_ms", "tiles"} of the proposal calls since the last
        reset_stats(): the time between two events around their launch
        sequences and the frame-pair tiles they computed, n (n - 1) / 2 a call
        (sift_mi_pair_counters)."""
        ms, tiles = ctypes.c_double(), ctypes.c_uint64()
        check(lib().sift_mi_pair_counters(self._h, ctypes.byref(ms), ctypes.byref(tiles)))
        return {"kernel_ms": ms.value, "tiles": tiles.value}

    # -- spread-limited keypoints (LABELLED EXTENSION: not in the crate) -----------
    def select_spread_device(self, d_kps_ptr, d_desc_ptr, offsets, limit, c=0.9, radius2=True):
        """LABELLED EXTENSION: up to `limit` keypoints per segment of a device
        arena, spread over the frame by adaptive non-maximal suppression
        (sift_mi_select_spread_device; the rule is tests/select_ref.py's).  A
        row's squared radius is its unfused f32 squared distance to the
        nearest row j of its segment with response_i < c * response_j
        (0 < c <= 1), inf without one; the min(rows, limit) rows with the
        largest radius are kept (the lower row first among equals), in
        ascending row order.  d_desc_ptr may be None (keypoints only).
        Returns a Selection; radius2=False leaves its radius2 None.  Where
        features_limit keeps the strongest responses wherever they cluster,
        this keeps the keypoints a homography, a fundamental matrix or a
        track set wants: all over the frame."""
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        if offs.ndim != 1 or len(offs) < 1 or (offs < 0).any():
            raise ValueError("offsets: n_segs + 1 non-negative row numbers")
        n = len(offs) - 1
        limit = int(limit)
        if not 0 <= limit <= 0xFFFFFFFF:
            raise ValueError("limit must fit 32 bits")
        c_offs = (ctypes.c_size_t * len(offs))(*[int(v) for v in offs])
        sel = (ctypes.c_size_t * len(offs))()
        lens = np.maximum(np.diff(offs), 0)
        cap = int(np.minimum(lens, limit).sum())
        rows = np.zeros(max(cap, 1), np.uint32)
        r2 = np.zeros(max(int(offs[-1] - offs[0]), 1), np.float32) if radius2 else None
        prm = _lib.SelectParams(limit, float(c))
        check(lib().sift_mi_select_spread_device(self._h, ctypes.c_void_p(d_kps_ptr), ctypes.c_void_p(d_desc_ptr),
                                                 c_offs, n, ctypes.byref(prm), sel, rows.ctypes.data, cap,
                                                 r2.ctypes.data if radius2 else None))
        kp, desc, k = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        check(lib().sift_mi_selected_results(self._h, ctypes.byref(kp), ctypes.byref(desc), ctypes.byref(k)))
        return Selection(np.array(sel[:], dtype=np.int64), rows[:k.value],
                         r2[:max(int(offs[-1] - offs[0]), 0)] if radius2 else None, kp.value, desc.value)

    def select_frames(self, offsets, limit, c=0.9, radius2=True):
        """select_spread_device on the results the last
        sift_batch_device(..., fetch=False) left in HBM (which stay as they
        are): sel = select_frames(offs, 2000), then e.g.
        match_pairs_device(sel.d_desc_ptr, sel.offsets, pairs)."""
        d_kps, d_desc, n = self.device_results()
        if int(offsets[-1]) > n:
            raise ValueError("offsets reach beyond the device results")
        return self.select_spread_device(d_kps, d_desc, offsets, limit, c, radius2)

    def select_keypoints(self, kps, limit, c=0.9):
        """The one-frame form on host keypoints (sift_mi_select_keypoints):
        kps an (n, 5) f32 keypoint array (SiftResult.keypoints_array; x, y and
        response are read).  Returns (rows uint32 ascending, radius2 f32 (n,))."""
        k = np.ascontiguousarray(kps, dtype=np.float32).reshape(-1, 5)
        limit = int(limit)
        if not 0 <= limit <= 0xFFFFFFFF:
            raise ValueError("limit must fit 32 bits")
        cap = min(len(k), limit)
        buf = k if len(k) else np.zeros((1, 5), np.float32)
        rows = np.zeros(max(cap, 1), np.uint32)
        r2 = np.zeros(max(len(k), 1), np.float32)
        n_rows = ctypes.c_size_t()
        prm = _lib.SelectParams(limit, float(c))
        check(lib().sift_mi_select_keypoints(self._h, buf.ctypes.data, len(k), ctypes.byref(prm), rows.ctypes.data, cap,
                                             ctypes.byref(n_rows), r2.ctypes.data))
        return rows[:n_rows.value], r2[:len(k)]

    def select_counters(self):
        """{"kernel_ms", "pair_tests"} of the select calls since the last
        reset_stats(): the time between two events around their launch
        sequences and the (row, candidate) tests they made, the sum of rows^2
        over a call's segments (sift_mi_select_counters)."""
        ms, tests = ctypes.c_double(), ctypes.c_uint64()
        check(lib().sift_mi_select_counters(self._h, ctypes.byref(ms), ctypes.byref(tests)))
        return {"kernel_ms": ms.value, "pair_tests": tests.value}

    # -- the input step ------------------------------
    def decode_jpeg(self, data):
        """Baseline JPEG bytes -> (h, w) u8 luma, as the reference makes its
        inputs: `image::open(..)` (zune-jpeg) then `.grayscale()`
        (examples/run-sift.rs:8, src/lib.rs:1012).  Entropy decoding on the
        host, IDCT / upsampling / colour on the GPU."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        w, h = jpeg_dims(buf)
        out = np.empty((h, w), np.uint8)
        check(lib().sift_mi_decode_jpeg(self._h, buf.ctypes.data, len(buf), out.ctypes.data, w, 0))
        return out

    def decode_jpeg_device(self, data, out_ptr, out_stride):
        """The same into device memory (e.g. a torch.uint8 CUDA tensor's
        data_ptr(), row stride in bytes), ordered on the context stream."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        check(lib().sift_mi_decode_jpeg(self._h, buf.ctypes.data, len(buf), out_ptr, out_stride, 1))

    def decode_jpeg_batch_device(self, datas, out_ptr, frame_pitch, row_stride, threads=0):
        """Equal-size JPEGs -> device frames (frame i at out_ptr + i *
        frame_pitch), ready for sift_batch_device; host threads decode the
        entropy-coded data."""
        bufs = [np.frombuffer(bytes(d), dtype=np.uint8) for d in datas]
        ptrs = (ctypes.c_void_p * max(1, len(bufs)))(*[b.ctypes.data for b in bufs])
        lens = (ctypes.c_size_t * max(1, len(bufs)))(*[len(b) for b in bufs])
        check(lib().sift_mi_decode_jpeg_batch(self._h, ptrs, lens, len(bufs), out_ptr, frame_pitch, row_stride,
                                              int(threads)))

    def sift_jpeg(self, data, features_limit=None):
        """`sift(image::open(path)?.grayscale())` of examples/run-sift.rs on
        JPEG bytes."""
        return self.sift(self.decode_jpeg(data), features_limit)

    # -- Processing ops (src/lib.rs:86-90) ---------------------------------
    def gaussian_blur(self, img, sigma):
        a = _f32_image(img)
        out = np.empty_like(a)
        check(lib().sift_mi_gaussian_blur(self._h, a.ctypes.data, a.shape[1], a.shape[0], float(sigma),
                                          out.ctypes.data))
        return out

    def resize_linear(self, img, width, height):
        a = _f32_image(img)
        out = np.empty((height, width), np.float32)
        check(lib().sift_mi_resize_linear(self._h, a.ctypes.data, a.shape[1], a.shape[0], width, height,
                                          out.ctypes.data))
        return out

    def resize_nearest(self, img, width, height):
        a = _f32_image(img)
        out = np.empty((height, width), np.float32)
        check(lib().sift_mi_resize_nearest(self._h, a.ctypes.data, a.shape[1], a.shape[0], width, height,
                                           out.ctypes.data))
        return out


class PrecomputedImages:
    """src/lib.rs:123-128: scale_space[o] is (6, h, w) f32, dog[o] (5, h, w)."""

    def __init__(self, ctx, n_octaves, generation):
        self._ctx = ctx
        self.n_octaves = n_octaves
        self._gen = generation

    def _check(self):
        if self._gen != self._ctx._generation:
            raise SiftMiError(-6, "PrecomputedImages superseded by a later precompute on this context")

    def dims(self, o):
        w, h = ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().sift_mi_octave_dims(self._ctx._h, o, ctypes.byref(w), ctypes.byref(h)))
        return w.value, h.value

    def scale_space_octave(self, o):
        self._check()
        w, h = self.dims(o)
        out = np.empty((6, h, w), np.float32)
        check(lib().sift_mi_read_scale_space(self._ctx._h, o, out.ctypes.data))
        return out

    def dog_octave(self, o):
        self._check()
        w, h = self.dims(o)
        out = np.empty((5, h, w), np.float32)
        check(lib().sift_mi_read_dog(self._ctx._h, o, out.ctypes.data))
        return out

    @property
    def scale_space(self):
        return [self.scale_space_octave(o) for o in range(self.n_octaves)]

    @property
    def dog(self):
        return [self.dog_octave(o) for o in range(self.n_octaves)]


# ---------------------------------------------------------------------------
# Processing backends (src/lib.rs:86-90, :993-1007; src/opencv_processing.rs)
# ---------------------------------------------------------------------------
class Processing:
    profile = None

    @classmethod
    def gaussian_blur(cls, img, sigma):
        return default_context(processing=cls).gaussian_blur(img, sigma)

    @classmethod
    def resize_linear(cls, img, width, height):
        return default_context(processing=cls).resize_linear(img, width, height)

    @classmethod
    def resize_nearest(cls, img, width, height):
        return default_context(processing=cls).resize_nearest(img, width, height)


class OpenCVProcessing(Processing):
    """cv::GaussianBlur / cv::resize arithmetic (src/opencv_processing.rs:38-74)."""
    profile = PROFILE_OPENCV


class ImageprocProcessing(Processing):
    """imageproc gaussian_blur_f32 / image::imageops::resize arithmetic
    (src/lib.rs:993-1007): the crate's default backend.  Restated from
    imageproc 0.25.0 / image 0.25.2 (not in the reference tree); parity
    against the reference is unpinned (no reference test runs it)."""
    profile = PROFILE_IMAGEPROC


_tls = threading.local()


def default_context(device=0, processing=None):
    processing = processing or ImageprocProcessing
    cache = getattr(_tls, "ctx", None)
    if cache is None:
        cache = _tls.ctx = {}
    key = (device, processing.profile)
    if key not in cache:
        cache[key] = Context(device, processing)
    return cache[key]


def sift(img, features_limit=None):
    """src/lib.rs:71: sift_with_processing::<ImageprocProcessing>."""
    return default_context(processing=ImageprocProcessing).sift(img, features_limit)


def sift_with_processing(processing, img, features_limit=None):
    """src/lib.rs:76"""
    return default_context(processing=processing).sift(img, features_limit)


def precompute_images(processing, img):
    """src/lib.rs:131"""
    return default_context(processing=processing).precompute_images(img)


def sift_with_precomputed(pre, features_limit=None):
    """src/lib.rs:147"""
    return pre._ctx.sift_with_precomputed(pre, features_limit)


def compute_descriptor(img, x, y, scale, orientation):
    """src/lib.rs:785"""
    return default_context().compute_descriptor(img, x, y, scale, orientation)


def jpeg_dims(data):
    """(width, height) of a baseline JPEG from its headers (host only)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    w, h = ctypes.c_uint32(), ctypes.c_uint32()
    check(lib().sift_mi_jpeg_dims(buf.ctypes.data, len(buf), ctypes.byref(w), ctypes.byref(h)))
    return w.value, h.value


def decode_jpeg(data):
    return default_context().decode_jpeg(data)


def match_descriptors(query, train, cross_check=True, ratio=None):
    """examples/sift-match.rs:30-35: BFMatcher(NORM_L2, crossCheck).match
    (`ratio`: Lowe's ratio test, a labelled extension)."""
    return default_context().match_descriptors(query, train, cross_check, ratio)


def match_neighbors(query, train):
    """LABELLED EXTENSION: BFMatcher(NORM_L2).knnMatch(query, train, 2)."""
    return default_context().match_neighbors(query, train)


def match_pairs_device(d_desc_ptr, offsets, pairs, ratio=None, cross_check=True):
    """Context.match_pairs_device on the default context."""
    return default_context().match_pairs_device(d_desc_ptr, offsets, pairs, ratio, cross_check)


def match_frames(offsets, pairs, ratio=None, cross_check=True):
    """Context.match_frames on the default context (its last
    sift_batch_device(..., fetch=False) results)."""
    return default_context().match_frames(offsets, pairs, ratio, cross_check)


def verify_pairs_device(d_kps_ptr, offsets, pairs, matches, threshold=3.0, iterations=1024, seed=0, refit_rounds=2,
                        model="homography", sampling="uniform", quality=None):
    """LABELLED EXTENSION: Context.verify_pairs_device on the default context."""
    return default_context().verify_pairs_device(d_kps_ptr, offsets, pairs, matches, threshold, iterations, seed,
                                                 refit_rounds, model, sampling, quality)


def verify_frames(offsets, pairs, matches, threshold=3.0, iterations=1024, seed=0, refit_rounds=2,
                  model="homography", sampling="uniform", quality=None):
    """LABELLED EXTENSION: Context.verify_frames on the default context (its
    last sift_batch_device(..., fetch=False) results)."""
    return default_context().verify_frames(offsets, pairs, matches, threshold, iterations, seed, refit_rounds, model,
                                           sampling, quality)


def verify_matches(kps_q, kps_t, matches, threshold=3.0, iterations=1024, seed=0, refit_rounds=2, model="homography",
                   sampling="uniform", quality=None):
    """LABELLED EXTENSION: Context.verify_matches on the default context."""
    return default_context().verify_matches(kps_q, kps_t, matches, threshold, iterations, seed, refit_rounds, model,
                                            sampling, quality)


def match_pairs_guided_device(d_desc_ptr, d_kps_ptr, offsets, pairs, models, threshold=3.0, model="homography",
                              ratio=None, max_distance=None, cross_check=True):
    """LABELLED EXTENSION: Context.match_pairs_guided_device on the default context."""
    return default_context().match_pairs_guided_device(d_desc_ptr, d_kps_ptr, offsets, pairs, models, threshold,
                                                       model, ratio, max_distance, cross_check)


def match_frames_guided(offsets, pairs, models, threshold=3.0, model="homography", ratio=None, max_distance=None,
                        cross_check=True):
    """LABELLED EXTENSION: Context.match_frames_guided on the default context
    (its last sift_batch_device(..., fetch=False) results)."""
    return default_context().match_frames_guided(offsets, pairs, models, threshold, model, ratio, max_distance,
                                                 cross_check)


def match_guided(desc_q, kps_q, desc_t, kps_t, model_matrix, threshold=3.0, model="homography", ratio=None,
                 max_distance=None, cross_check=True):
    """LABELLED EXTENSION: Context.match_guided on the default context."""
    return default_context().match_guided(desc_q, kps_q, desc_t, kps_t, model_matrix, threshold, model, ratio,
                                          max_distance, cross_check)


def build_tracks_device(d_kps_ptr, offsets, pairs, matches, keep=None, min_length=2, conflicts="flag"):
    """LABELLED EXTENSION: Context.build_tracks_device on the default context."""
    return default_context().build_tracks_device(d_kps_ptr, offsets, pairs, matches, keep, min_length, conflicts)


def track_frames(offsets, pairs, matches, keep=None, min_length=2, conflicts="flag"):
    """LABELLED EXTENSION: Context.track_frames on the default context (its
    last sift_batch_device(..., fetch=False) results)."""
    return default_context().track_frames(offsets, pairs, matches, keep, min_length, conflicts)


def propose_pairs_device(d_desc_ptr, d_kps_ptr, offsets, subset=128, ratio=0.8, min_matches=8, max_partners=0):
    """LABELLED EXTENSION: Context.propose_pairs_device on the default context."""
    return default_context().propose_pairs_device(d_desc_ptr, d_kps_ptr, offsets, subset, ratio, min_matches,
                                                  max_partners)


def propose_frames(offsets, subset=128, ratio=0.8, min_matches=8, max_partners=0):
    """LABELLED EXTENSION: Context.propose_frames on the default context (its
    last sift_batch_device(..., fetch=False) results)."""
    return default_context().propose_frames(offsets, subset, ratio, min_matches, max_partners)


def pair_counters():
    """LABELLED EXTENSION: Context.pair_counters on the default context."""
    return default_context().pair_counters()


def select_spread_device(d_kps_ptr, d_desc_ptr, offsets, limit, c=0.9, radius2=True):
    """LABELLED EXTENSION: Context.select_spread_device on the default context."""
    return default_context().select_spread_device(d_kps_ptr, d_desc_ptr, offsets, limit, c, radius2)


def select_frames(offsets, limit, c=0.9, radius2=True):
    """LABELLED EXTENSION: Context.select_frames on the default context (its
    last sift_batch_device(..., fetch=False) results)."""
    return default_context().select_frames(offsets, limit, c, radius2)


def select_keypoints(kps, limit, c=0.9):
    """LABELLED EXTENSION: Context.select_keypoints on the default context."""
    return default_context().select_keypoints(kps, limit, c)


def select_counters():
    """LABELLED EXTENSION: Context.select_counters on the default context."""
    return default_context().select_counters()


def stable_sort_xy_size(keypoints_array):
    """Order of the reference test's snapshots (src/lib.rs:1020-1030): stable
    sort by (x, y, size)."""
    k = np.asarray(keypoints_array)
    if not len(k):
        return np.zeros(0, np.int64)
    return np.lexsort((k[:, 2], k[:, 1], k[:, 0]))


def key_fields(keys):
    """Decode emission keys (include/sift_mi.h sift_mi_fetch_keys)."""
    k = np.asarray(keys, dtype=np.uint64)
    f = lambda s, b: ((k >> np.uint64(s)) & np.uint64((1 << b) - 1)).astype(np.int64)
    return {"frame": f(42, 22), "octave": f(38, 4), "s_init": f(36, 2), "y_init": f(21, 15),
            "x_init": f(6, 15), "peak": f(0, 6)}
