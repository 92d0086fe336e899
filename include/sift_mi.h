/*
 * sift_mi.h -- C ABI of the MI355X-native SIFT hot path (libsift_mi.so).
 *
 * Drop-in boundary for tnibler/sift-features (src/lib.rs @ 2024-10-22).
 * Plain pointers and sizes only (no HIP, torch or Rust types), so that the
 * crate's `sift()` can be re-implemented as a thin `extern "C"` shim (see
 * INTEGRATION.md for the Rust binding a maintainer would add).
 *
 * Every entry point names the reference interface it replaces (file:line).
 * All functions return 0 (SIFT_MI_OK) on success or a negative
 * sift_mi_status; sift_mi_last_error() describes the last failure of the
 * calling thread.  The reference is infallible (it panics); the Rust shim
 * panics with sift_mi_last_error() to keep that signature.
 *
 * Threading: a context is not thread-safe; use one context per thread (and
 * per GPU).  Distinct contexts run concurrently.
 * Ownership: inputs are borrowed for the duration of a call.  Results live
 * in context-owned buffers until the next extraction call or destroy.
 *
 * Call sequence.  A context remembers what its last PRODUCING call left, and
 * that alone decides the return code of a later call; five values:
 *   where          none | host | device: where the last result's rows are
 *   n              their number
 *   pyramid        the planes of sift_mi_precompute are in the context
 *   batch_readback the last extraction ran as one chunk (one frame, or
 *                  sift_mi_set_chunk >= its frames, and no restricted row
 *                  band), so its planes can be read back
 *   keep           the sift_mi_set_keep_on_device setting
 * A new context has where = none, n = 0 and the three flags 0.
 *
 *   call                              needs            on success
 *   sift_mi_extract,                  -                where = host, pyramid = 0,
 *   sift_mi_extract_batch                              batch_readback = the call
 *     (host frames)                                    ran as one chunk
 *   sift_mi_extract_batch_device      -                where = keep ? device : host,
 *                                                      otherwise as above
 *   sift_mi_precompute                -                pyramid = 1, where = none,
 *                                                      batch_readback = 0
 *   sift_mi_sift_with_precomputed     pyramid          where = host, batch_readback
 *                                                      = 0, pyramid stays
 *   sift_mi_fetch, sift_mi_fetch_keys where == host    unchanged
 *   sift_mi_device_results            where == device  unchanged
 *   sift_mi_octave_dims,              pyramid          unchanged
 *   sift_mi_read_scale_space,
 *   sift_mi_read_dog
 *   sift_mi_batch_octave_dims,        batch_readback   unchanged
 *   sift_mi_read_batch_scale_space
 *   sift_mi_set_keep_on_device        -                keep only; where does not move
 *   sift_mi_set_max_octaves           -                pyramid = 0, batch_readback = 0
 *
 *   - A call whose "needs" is unmet returns SIFT_MI_ESTATE and changes nothing.
 *   - A call refused for its arguments, before any buffer is touched, changes
 *     nothing: every SIFT_MI_EINVAL of the four producing calls' own argument
 *     checks (null pointer, zero size, stride < width, a frame above 16384 px,
 *     too many frames, features_limit while n_bands > 1), and a cap below n in
 *     the fetch calls.  "needs" is checked before the arguments.
 *   - A producing call that fails later (the plan was replaced, an arena or a
 *     stage buffer rewritten: SIFT_MI_ENOMEM, SIFT_MI_EHIP, SIFT_MI_EUNSUPPORTED)
 *     leaves where = none, pyramid = 0, batch_readback = 0.  The host-frame
 *     calls and sift_mi_precompute copy their frames to a staging buffer
 *     before that point: a failure of that copy (a null pointer inside
 *     `frames` included) changes nothing.
 *   - Every other call (the remaining setters, the match / verify / track /
 *     pair / select calls, the JPEG and op-level calls, the statistics) neither
 *     needs nor changes any of the five.
 * Where the last result lives is a fact recorded by the call that produced it:
 * sift_mi_set_keep_on_device chooses the destination of LATER
 * sift_mi_extract_batch_device calls and nothing else.  Host-frame calls and
 * sift_mi_sift_with_precomputed always deliver to the host, under either
 * setting.  (sift-features_amd/csrc/result_state.h is this rule as code;
 * tests/call_model.py restates it.)
 */
#ifndef SIFT_MI_H
#define SIFT_MI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIFT_MI_DESCRIPTOR_SIZE 128

/* src/lib.rs:48-56 `KeyPoint` (the Rust struct is not repr(C); the shim
 * converts field by field).  x, y, size are in input-image pixels (the
 * reference's final `* DELTA_MIN`, src/lib.rs:163-176, is applied). */
typedef struct {
    float x, y, size, angle, response;
} sift_mi_keypoint;

/* src/lib.rs:86-90 `trait Processing`: which blur / resize arithmetic the
 * pyramid uses.  OPENCV = `OpenCVProcessing` (src/opencv_processing.rs:38-74,
 * the backend the reference's golden snapshots pin).  IMAGEPROC =
 * `ImageprocProcessing` (src/lib.rs:993-1007), the crate's default for
 * `sift()`: imageproc 0.25 gaussian_blur_f32 + image 0.25 resize arithmetic,
 * restated (those crates are not in the reference tree and no reference test
 * runs this profile: parity unpinned). */
typedef enum { SIFT_MI_PROFILE_OPENCV = 0, SIFT_MI_PROFILE_IMAGEPROC = 1 } sift_mi_profile;

typedef enum {
    SIFT_MI_OK = 0,
    SIFT_MI_EINVAL = -1,      /* bad argument (null pointer, zero size, stride < width ...) */
    SIFT_MI_ENOMEM = -2,      /* device or host allocation failed */
    SIFT_MI_EHIP = -3,        /* HIP runtime error (message in sift_mi_last_error) */
    SIFT_MI_ENODEV = -4,      /* no usable gfx950 device */
    SIFT_MI_EUNSUPPORTED = -5,/* profile / feature not implemented */
    SIFT_MI_ESTATE = -6       /* call sequence error (e.g. fetch before extract) */
} sift_mi_status;

typedef struct sift_mi_ctx sift_mi_ctx;

/* Create a context on HIP device `device_ordinal`; owns one HIP stream and
 * pooled device buffers.  Fails with SIFT_MI_ENODEV on a non-gfx950 device. */
int sift_mi_create(int device_ordinal, sift_mi_profile profile, sift_mi_ctx** out);
void sift_mi_destroy(sift_mi_ctx* ctx);

/* Run subsequent work on an external hipStream_t (e.g. a torch side stream);
 * NULL restores the context-owned stream.
 *   Order: every kernel and copy of a later call -- also those the library
 *   runs on streams of its own (pipeline lane 1, the octave and descriptor
 *   streams, the result copies) -- is ordered after the work already enqueued
 *   on that stream when the call is made.  Frames, descriptors or keypoints
 *   produced by a kernel on the stream can be handed over without a host
 *   synchronisation, and an output buffer (sift_mi_decode_jpeg,
 *   sift_mi_decode_jpeg_batch) is written after earlier writes to it there.
 *   Completion: every entry point, without exception, returns after its
 *   results are complete.  That includes results left in device memory
 *   (sift_mi_device_results after a keep_on_device call, the frames the JPEG
 *   decode calls write): work enqueued on any stream after the call returns
 *   may read them.
 *   Lifetime: the stream must outlive the context, or be reset to NULL before
 *   it is destroyed (sift_mi_destroy synchronises the stream in force).
 *   NULL is the context's own stream, created hipStreamNonBlocking: it does
 *   not synchronise with the legacy default stream (handle 0).  A caller whose
 *   work runs on the legacy default stream must synchronise before the call,
 *   or use a side stream and pass that.
 *   With SIFT_MI_PATH_GRAPH the stream is part of the graph's key: after a
 *   change of stream the next identical call is captured anew. */
int sift_mi_set_stream(sift_mi_ctx* ctx, void* hip_stream);

/* Images per internal pipeline chunk for batch calls (0 = automatic). */
int sift_mi_set_chunk(sift_mi_ctx* ctx, uint32_t images_per_chunk);

/* ---- src/lib.rs:71 `sift(img, features_limit) -> SiftResult` ------------
 * `pixels`: row-major u8 GrayImage, `row_stride` >= width bytes per row.
 * features_limit < 0 == None.  With a limit the result is ordered by
 * response, descending (src/lib.rs:156-161); ties keep emission order (the
 * reference's sort_unstable_by leaves them unspecified).
 * Writes the keypoint count to *n_keypoints; fetch with sift_mi_fetch. */
int sift_mi_extract(sift_mi_ctx* ctx, const uint8_t* pixels, uint32_t width, uint32_t height,
                    size_t row_stride, int64_t features_limit, size_t* n_keypoints);

/* Copy the last result: `kps[cap]`, `desc[cap * 128]` (row i <-> keypoint i,
 * the (n,128) C-order `Array2<u8>` of SiftResult::descriptors).  Either
 * pointer may be NULL.  cap must be >= the result size (SIFT_MI_EINVAL).
 * Needs where == host ("Call sequence" above): SIFT_MI_ESTATE before any
 * producing call, after sift_mi_precompute, after a failed producing call and
 * after a device-kept batch, whatever sift_mi_set_keep_on_device says now. */
int sift_mi_fetch(sift_mi_ctx* ctx, sift_mi_keypoint* kps, uint8_t* desc, size_t cap);

/* Emission keys of the last result, for parity checks: bits
 * [42,64) image, [38,42) octave, [36,38) initial scale, [21,36) initial y,
 * [6,21) initial x, [0,6) orientation peak (x/y in octave pixels; octave 0
 * is the 2x seed, so frames up to 16384 px fit the 15-bit fields) -- the reference's emission order
 * (src/lib.rs:281-294, :324-332, :397-431). */
int sift_mi_fetch_keys(sift_mi_ctx* ctx, uint64_t* keys, size_t cap);

/* ---- batch of equal-size frames (throughput path; one `sift()` per frame)
 * `offsets[n+1]` receives the per-frame ranges in the concatenated result. */
int sift_mi_extract_batch(sift_mi_ctx* ctx, const uint8_t* const* frames, uint32_t n, uint32_t width,
                          uint32_t height, size_t row_stride, int64_t features_limit, size_t* offsets);

/* Same, frames already resident in device memory: frame i starts at
 * d_frames + i * frame_pitch (bytes).  The timed path of bench.py. */
int sift_mi_extract_batch_device(sift_mi_ctx* ctx, const uint8_t* d_frames, size_t frame_pitch, uint32_t n,
                                 uint32_t width, uint32_t height, size_t row_stride, int64_t features_limit,
                                 size_t* offsets);

/* Descriptor accumulation order.  0 (default): lane-private histograms summed
 * per bin -- components within +-1 of the reference.  1: bins accumulated in
 * the reference's sequential sample order (src/lib.rs:883-948) -- bit-exact
 * descriptors, slower.  Keypoints are identical in both modes. */
int sift_mi_set_exact_descriptors(sift_mi_ctx* ctx, int exact);

/* LABELLED EXTENSION (not in the crate): cap the octave count at max_octaves
 * (0 = the crate's formula round(log2(min(2W, 2H)) - 2) + 1, src/lib.rs:133-134,
 * the default).  The kept octaves are computed exactly as without the cap.
 * With features_limit None the result is the uncapped result's keypoints of
 * octaves < max_octaves (a prefix of the emission order).  With a limit, the
 * cap applies first: the limit ranks the capped keypoint set (src/lib.rs:156-161
 * on the prefix), which is not in general a subset of the uncapped limited
 * result.  For the "5 octaves" / "7 octaves" wording of BASELINE.json's
 * configs; parity runs leave it at 0. */
int sift_mi_set_max_octaves(sift_mi_ctx* ctx, int max_octaves);

/* Batch pipeline lanes: 2 (default) runs consecutive chunks on two streams
 * with their own pyramid arenas, so one chunk's kernels overlap the other's;
 * 1 runs the chunks one after another on the context's stream (half the
 * device memory; used to time kernels in isolation). */
int sift_mi_set_pipeline_lanes(sift_mi_ctx* ctx, int lanes);

/* Row band of the keypoint stages, for splitting ONE large frame across
 * contexts / GPUs (replaces nothing in the reference,
 * whose sift() is whole-frame: src/lib.rs:71-81).  With n_bands > 1,
 * detection (and so refinement, orientation and descriptors) covers only
 * octave rows [H_o*band/n_bands, H_o*(band+1)/n_bands) of each octave o,
 * and the pyramid is computed only on those rows plus the halos they read
 * (a refinement reaching beyond them re-runs the call on the whole pyramid:
 * sift_mi_stats.band_reruns; OpenCV profile, else the whole pyramid).  The bands
 * partition every octave's candidate rows, so the union of the n_bands
 * results, ordered by emission key (sift_mi_fetch_keys), is exactly the
 * whole-frame result.  features_limit is rejected (SIFT_MI_EINVAL) while
 * n_bands > 1: it ranks the whole frame's keypoints, so apply it after the
 * merge.  Default band 0 of 1 (the whole frame). */
int sift_mi_set_row_band(sift_mi_ctx* ctx, uint32_t band, uint32_t n_bands);

/* Skip the device->host copy of results in later
 * sift_mi_extract_batch_device calls (their results stay in device memory;
 * see sift_mi_device_results).  Default 0 = copy.  Only a setting: the last
 * result stays where its call put it, and sift_mi_fetch /
 * sift_mi_device_results go on answering for that call.  Host-frame calls
 * (sift_mi_extract, sift_mi_extract_batch) and sift_mi_sift_with_precomputed
 * deliver to the host under either value. */
int sift_mi_set_keep_on_device(sift_mi_ctx* ctx, int keep);

/* Device pointers of the last result, when a sift_mi_extract_batch_device
 * call under keep_on_device = 1 produced it (where == device, "Call sequence"
 * above; SIFT_MI_ESTATE otherwise, with the outputs untouched): the
 * keypoints and descriptors of every frame, concatenated in frame order
 * (frame i at offsets[i] .. offsets[i+1]); valid until the next producing
 * call (extraction, precompute, sift_with_precomputed) or destroy: the match
 * calls only read them, so several sift_mi_match_pairs_device calls may
 * follow one extraction. */
int sift_mi_device_results(sift_mi_ctx* ctx, const sift_mi_keypoint** d_kps, const uint8_t** d_desc, size_t* n);

/* Validation read-back (extension, not the crate): the Gaussian planes
 * G_0..G_5 of octave `octave` of frame `frame` of the last batch / sift()
 * call, as that call's pyramid left them in the context's arena -- (6, h, w)
 * f32 like sift_mi_read_scale_space, with (w, h) from
 * sift_mi_batch_octave_dims; `out_floats` is the capacity of `out`
 * (SIFT_MI_EINVAL below 6 * w * h).  Valid only when the last extraction ran
 * as one chunk (one frame, or sift_mi_set_chunk >= its frames) and until the
 * next producing call (precompute and sift_with_precomputed included) or
 * sift_mi_set_max_octaves: batch_readback of "Call sequence" above;
 * SIFT_MI_ESTATE otherwise.
 * Lets tests check the batch path's planes (which no DoG is materialised
 * for) against precompute_images. */
int sift_mi_batch_octave_dims(sift_mi_ctx* ctx, size_t octave, uint32_t* width, uint32_t* height);
int sift_mi_read_batch_scale_space(sift_mi_ctx* ctx, uint32_t frame, size_t octave, float* out, size_t out_floats);

/* Kernel-path switches (test / diagnostic, not configuration).  The default
 * of every option is the product path; each alternative computes the same
 * bits through a different kernel family, so the tests can hold every family
 * against the oracle.  Per context (no environment variables, no process-wide
 * state); waits for the context's work in flight.  SIFT_MI_EINVAL for an
 * unknown option or a value out of range. */
typedef enum {
    SIFT_MI_PATH_TILE_BLUR = 0,    /* 1: one-tile-per-workgroup blurs everywhere (default 0) */
    SIFT_MI_PATH_PAIR_BLUR = 1,    /* 0: no two-blur kernels (default 1) */
    SIFT_MI_PATH_SEED_PAIR = 2,    /* 0: seed and blur 1 as two launches (default 1) */
    SIFT_MI_PATH_TAIL = 3,         /* 0: per-blur launches for the small octaves (default 1) */
    SIFT_MI_PATH_FUSED_DETECT = 4, /* 0: blur 5 and the extremum scan apart; 2: fused wherever it
                                      applies, at 32-row segments (default 1: where it fills the chip) */
    SIFT_MI_PATH_EARLY = 5,        /* 0: one-chunk calls detect every octave after the tail (default 1) */
    SIFT_MI_PATH_DESC_FIRST = 6,   /* 0: one-frame calls order, then describe (default 1) */
    SIFT_MI_PATH_GRAPH = 7,        /* 1: identical single-chunk calls replayed as a HIP graph (default 0) */
    SIFT_MI_PATH_BAND_DRIFT = 8,   /* row bands: accepted refinement drift, -41..24 rows (default 24;
                                      smaller values force the whole-pyramid re-run) */
    SIFT_MI_PATH_BOUND_SHRINK = 9, /* k >= 1: first-chunk stage bounds / k (default 1; > 1 forces the
                                      bound-overflow re-run) */
    /* 10: retired (the round-5 split tail kernel, removed in round 6); setting it returns
       SIFT_MI_EINVAL */
    SIFT_MI_PATH_LARGE_FIRST = 11, /* 0: one-chunk calls orient the extrema in refinement order, not
                                      those with large windows first (default 1) */
    SIFT_MI_PATH_ONESWEEP = 12,    /* the emission-order sorts with rocprim's Onesweep radix sort: 1 at
                                      every size, 0 never, 2 from 524288 keys (default 0) */
    SIFT_MI_PATH_BD_PAIR = 13,     /* the fused blur 5 + extremum scan with two column strips per lane
                                      (packed f32): 1 (default) / 2 its two loop forms, 0 the one-column
                                      kernel */
    SIFT_MI_PATH_BD_WAVES = 14,    /* the pair kernel's fewest waves per launch when choosing its row
                                      segments, 1024..65536 */
    SIFT_MI_PATH_CHUNK_MODE = 15,  /* automatic chunking: 1 (default) as few chunks as ~64 GB of pyramid
                                      (counted at 44 B per octave pixel) and ~1062 M seed pixels per chunk
                                      allow (128 x 1080p: one chunk); 0 at least two chunks per
                                      multi-frame call (both pipeline lanes busy), <= ~32 GB / ~531 M
                                      seed pixels each (rounds 1-5).  Either way a chunk is capped at
                                      40% of the device memory the context could use */
    SIFT_MI_PATH_GUIDED_CULL = 16  /* guided matcher: 1 (default) a wave whose 64 x 64 block of a tile holds
                                      no admissible element skips its loads and MFMAs; 0 every wave runs them.
                                      The same bits either way (a diagnostic, not a tuning knob) */
} sift_mi_path_option;
int sift_mi_set_path_option(sift_mi_ctx* ctx, int option, int value);

/* ---- src/lib.rs:123-143 `precompute_images` / `PrecomputedImages` ------- */
int sift_mi_precompute(sift_mi_ctx* ctx, const uint8_t* pixels, uint32_t width, uint32_t height,
                       size_t row_stride, size_t* n_octaves);
/* The three read calls need `pyramid` of "Call sequence" above (SIFT_MI_ESTATE). */
int sift_mi_octave_dims(sift_mi_ctx* ctx, size_t octave, uint32_t* width, uint32_t* height);
/* scale_space[octave]: (6, h, w) f32; dog[octave]: (5, h, w) f32 */
int sift_mi_read_scale_space(sift_mi_ctx* ctx, size_t octave, float* out);
int sift_mi_read_dog(sift_mi_ctx* ctx, size_t octave, float* out);

/* ---- src/lib.rs:147 `sift_with_precomputed(&PrecomputedImages, limit)` --
 * On the planes of the last sift_mi_precompute (SIFT_MI_ESTATE when an
 * extraction, sift_mi_set_max_octaves or a failed call has ended them);
 * the result goes to the host: fetch with sift_mi_fetch.  May be called
 * repeatedly on one precompute. */
int sift_mi_sift_with_precomputed(sift_mi_ctx* ctx, int64_t features_limit, size_t* n_keypoints);

/* ---- src/lib.rs:785 `compute_descriptor(img, x, y, scale, orientation)` -
 * `img`: host f32 image (h, w); writes 128 bytes. */
int sift_mi_compute_descriptor(sift_mi_ctx* ctx, const float* img, uint32_t width, uint32_t height, float x,
                               float y, float scale, float orientation, uint8_t* out);

/* ---- src/lib.rs:86-90 `Processing` ops on host f32 images (op-level parity;
 * not the performance path) ------------------------------------------------ */
int sift_mi_gaussian_blur(sift_mi_ctx* ctx, const float* src, uint32_t width, uint32_t height, double sigma,
                          float* dst);
int sift_mi_resize_linear(sift_mi_ctx* ctx, const float* src, uint32_t width, uint32_t height, uint32_t dst_width,
                          uint32_t dst_height, float* dst);
int sift_mi_resize_nearest(sift_mi_ctx* ctx, const float* src, uint32_t width, uint32_t height, uint32_t dst_width,
                           uint32_t dst_height, float* dst);

/* ---- examples/sift-match.rs:30-35: cv::BFMatcher(NORM_L2, crossCheck)
 * .match(query, train) -- the step after the path.
 * query / train: (n, 128) u8 descriptor rows (SiftResult::descriptors).
 * distance = sqrt((float) exact integer L2^2); nearest = lowest index among
 * equal distances; cross_check != 0 keeps query i only when its nearest
 * train row's nearest query is i.  Matches are written in query order to
 * out[cap]; *n_matches = their count (SIFT_MI_EINVAL if cap is smaller, with
 * *n_matches set). */
typedef struct {
    int32_t query_idx, train_idx;
    float distance;
} sift_mi_match;
int sift_mi_match_descriptors(sift_mi_ctx* ctx, const uint8_t* query, size_t n_query, const uint8_t* train,
                              size_t n_train, int cross_check, sift_mi_match* out, size_t cap, size_t* n_matches);

/* LABELLED EXTENSION (the crate offers only BFMatcher(crossCheck).match):
 * cv::BFMatcher(NORM_L2).knnMatch(query, train, 2) -- per query its two
 * nearest train rows, ordered by (integer L2^2, index) ascending (OpenCV's
 * insertion rule: lowest index first among equals), distance as above.
 * out[n_query]; where a neighbour is absent (n_train < 2) train_idx is -1 and
 * distance +INFINITY. */
typedef struct {
    int32_t train_idx[2];
    float distance[2];
} sift_mi_neighbors;
int sift_mi_match_neighbors(sift_mi_ctx* ctx, const uint8_t* query, size_t n_query, const uint8_t* train,
                            size_t n_train, sift_mi_neighbors* out);

/* LABELLED EXTENSION: sift_mi_match_descriptors plus Lowe's ratio test on the
 * two nearest neighbours: a query is kept only if distance[0] < ratio *
 * distance[1] (f32, one multiply, strict), and rejected when it has no
 * second neighbour (n_train < 2).  ratio == 0: no ratio test (the result of
 * sift_mi_match_descriptors); otherwise 0 < ratio <= 1 (SIFT_MI_EINVAL for a
 * NaN, a negative value or one above 1).  With cross_check both tests must
 * pass. */
int sift_mi_match_ratio(sift_mi_ctx* ctx, const uint8_t* query, size_t n_query, const uint8_t* train,
                        size_t n_train, float ratio, int cross_check, sift_mi_match* out, size_t cap,
                        size_t* n_matches);

/* LABELLED EXTENSION: the same for many (query segment, train segment) pairs
 * of descriptors resident in device memory, in one launch sequence on the
 * context stream (returns once `out` is written; no allocation once the
 * context's scratch has grown to the call's size).  d_desc: (n, 128) u8 rows
 * in device memory, laid out like sift_mi_device_results' descriptors (any
 * device memory will do, 16-byte aligned); segment s is rows offsets[s] ..
 * offsets[s+1] (host array of n_segs + 1, e.g. the offsets of
 * sift_mi_extract_batch_device: one segment per frame).  Pair p matches the
 * rows of segment pairs[p].query_seg against those of pairs[p].train_seg; its
 * matches are out[pair_offsets[p] .. pair_offsets[p+1]), in query order, with
 * segment-relative indices; pairs come in the given order (pair_offsets is a
 * host array of n_pairs + 1).  An empty segment gives an empty range.  If
 * cap is too small the call returns SIFT_MI_EINVAL with
 * pair_offsets[n_pairs] set to the needed count.  SIFT_MI_EINVAL also for a
 * null argument, a bad ratio (as above), a pair index >= n_segs, decreasing
 * offsets, and a segment or a sum of segment lengths above 2^31 - 1.
 * The call only reads d_desc: it never invalidates the context's device
 * results, so any number of match calls may follow one extraction. */
typedef struct {
    uint32_t query_seg, train_seg;
} sift_mi_seg_pair;
int sift_mi_match_pairs_device(sift_mi_ctx* ctx, const uint8_t* d_desc, const size_t* offsets, uint32_t n_segs,
                               const sift_mi_seg_pair* pairs, uint32_t n_pairs, float ratio, int cross_check,
                               sift_mi_match* out, size_t cap, size_t* pair_offsets);

/* LABELLED EXTENSION (the crate has nothing like it; examples/sift-match.rs
 * stops at drawing the matches): geometric verification of matched pairs.
 * Per pair a RANSAC homography from `iterations` four-match samples, scored
 * by the count of matches within `threshold` px (in the train image) of the
 * projected query keypoint, then up to `refit_rounds` least-squares refits on
 * the inliers.  The rules -- the integer sampling (a function of seed,
 * hypothesis index and match count only: a pair's place in the call does not
 * matter), the orientation test of a sample, the f64 minimal solve, the f32
 * division-free score, ties to the lowest hypothesis, the refit's acceptance
 * -- are stated in tests/verify_ref.py, and without refits the result equals
 * that restatement bit for bit. */
typedef struct {
    float    threshold;     /* px in the train image, finite, > 0 */
    uint32_t iterations;    /* hypotheses per pair, 1..65536 */
    uint32_t seed;
    uint32_t refit_rounds;  /* 0..8 least-squares refits on the inliers */
} sift_mi_ransac_params;

typedef struct {
    float    h[9];            /* row-major, h[8] == 1: (x,y,1) of the query keypoint -> train; all 0 if no model */
    uint32_t n_matches;       /* the pair's match count */
    uint32_t n_inliers;       /* 0 if no model */
    int32_t  best_hypothesis; /* index of the winning sample, -1 if none was valid */
    uint32_t refits;          /* accepted refit rounds */
} sift_mi_homography;

/* d_kps, offsets, n_segs, pairs: as sift_mi_device_results and
 * sift_mi_match_pairs_device use them (keypoints of segment s at
 * d_kps[offsets[s] .. offsets[s+1])).  matches / pair_offsets: the host
 * arrays the match call wrote (pair p's matches at matches[pair_offsets[p] ..
 * pair_offsets[p+1]), segment-relative indices); the caller may have
 * filtered them.  The call uploads the matches, runs one launch sequence on
 * the context stream and returns once models[n_pairs] and
 * inliers[pair_offsets[n_pairs]] (1 = inlier, parallel to matches) are
 * written; no allocation once the context's scratch has grown to the call's
 * size.  It only reads d_kps and never invalidates the device results.
 * A pair with fewer than 4 matches or without a valid sample gets no model
 * (h all 0, n_inliers 0, best_hypothesis -1, a zero mask): a result, not an
 * error.  SIFT_MI_EINVAL, checked on the host before any device work (no
 * kernel sees an index outside its segment): a null argument, a threshold
 * that is not finite or <= 0, iterations of 0 or above 65536, refit_rounds
 * above 8, a pair index >= n_segs, decreasing offsets or pair_offsets, a
 * match index outside its pair's segment. */
int sift_mi_verify_pairs_device(sift_mi_ctx* ctx, const sift_mi_keypoint* d_kps, const size_t* offsets, uint32_t n_segs,
                                const sift_mi_seg_pair* pairs, uint32_t n_pairs,
                                const sift_mi_match* matches, const size_t* pair_offsets,
                                const sift_mi_ransac_params* params,
                                sift_mi_homography* models /* [n_pairs] */, uint8_t* inliers /* [pair_offsets[n_pairs]] */);

/* The one-pair form on host keypoints: uploads them and runs the same
 * kernels (matches / inliers may be null when n_matches is 0). */
int sift_mi_verify_matches(sift_mi_ctx* ctx, const sift_mi_keypoint* query_kps, size_t n_query,
                           const sift_mi_keypoint* train_kps, size_t n_train,
                           const sift_mi_match* matches, size_t n_matches,
                           const sift_mi_ransac_params* params, sift_mi_homography* model, uint8_t* inliers);

/* LABELLED EXTENSION like the homography above: epipolar verification of
 * matched pairs, the model for a moving camera in a 3-D scene.  Per pair a
 * RANSAC fundamental matrix F, (X, Y, 1) F (x, y, 1)^T = 0 for a query
 * keypoint (x, y) and its train keypoint (X, Y): `iterations` eight-match
 * samples, each solved by the 8-point method (f64, box-normalised
 * coordinates, Gaussian elimination with complete pivoting), scored by the
 * count of matches whose Sampson distance is <= `threshold` px, then up to
 * `refit_rounds` refits on the inliers (the smallest eigenvector of the
 * inliers' 9 x 9 moment matrix, made rank 2).  sift_mi_ransac_params is the
 * homography call's, its threshold read as the Sampson distance in px.  The
 * rules are stated in tests/epipolar_ref.py, and without refits the result
 * equals that restatement bit for bit.
 * F is rank 2, up to its f32 rounding, if and only if refits >= 1; with
 * refits == 0 it is the raw 8-point solution of the winning sample, which is
 * not.  Limits: a scene that is one plane (or a camera that only rotates)
 * satisfies a whole family of F, every match of the plane is an inlier of any
 * of them, and the homography call is the right tool there; an eight-match
 * sample is all inliers with probability share^8, so under uniform sampling
 * 1024 hypotheses suit inlier shares >= 0.5 and lower shares need more
 * iterations; the *_progressive calls below draw from the best-ranked matches
 * first and reach lower shares with the same count. */
typedef struct {
    float    f[9];            /* row-major, largest entry == 1; all 0 if no model */
    uint32_t n_matches;       /* the pair's match count */
    uint32_t n_inliers;       /* 0 if no model */
    int32_t  best_hypothesis; /* index of the winning sample, -1 if none was valid */
    uint32_t refits;          /* accepted refit rounds; F is rank 2 iff >= 1 */
} sift_mi_fundamental;

/* The arguments, the checks (SIFT_MI_EINVAL) and the guarantees of
 * sift_mi_verify_pairs_device / sift_mi_verify_matches.  A pair with fewer
 * than 8 matches or without a valid sample gets no model (f all 0, n_inliers
 * 0, best_hypothesis -1, a zero mask): a result, not an error. */
int sift_mi_verify_pairs_epipolar_device(sift_mi_ctx* ctx, const sift_mi_keypoint* d_kps, const size_t* offsets,
                                         uint32_t n_segs, const sift_mi_seg_pair* pairs, uint32_t n_pairs,
                                         const sift_mi_match* matches, const size_t* pair_offsets,
                                         const sift_mi_ransac_params* params,
                                         sift_mi_fundamental* models /* [n_pairs] */,
                                         uint8_t* inliers /* [pair_offsets[n_pairs]] */);
int sift_mi_verify_matches_epipolar(sift_mi_ctx* ctx, const sift_mi_keypoint* query_kps, size_t n_query,
                                    const sift_mi_keypoint* train_kps, size_t n_train,
                                    const sift_mi_match* matches, size_t n_matches,
                                    const sift_mi_ransac_params* params, sift_mi_fundamental* model, uint8_t* inliers);

/* LABELLED EXTENSION: the two verifications with progressive sampling (PROSAC:
 * Chum & Matas, "Matching with PROSAC", CVPR 2005).  Uniform sampling needs
 * share^k luck per hypothesis (k = 4 for the homography, 8 for the fundamental
 * matrix); here a pair's matches are ranked by a quality and hypothesis h draws
 * its sample from the best n_h of them, n_h growing with h, so the early
 * hypotheses come from the matches most likely to be right.  The rule is stated
 * in tests/prosac_ref.py, and without refits the result equals that
 * restatement bit for bit:
 *   Rank     match i of a pair has the key (u32 pattern of quality[i], i);
 *            ascending keys: the lower quality value first (a descriptor
 *            distance: lower is better), the lower index first among equals.
 *            quality is parallel to matches; null: matches[i].distance.
 *   Growth   f64, one rounding per operation.  N the pair's match count, T =
 *            iterations: T_k = T, for i = 0..k-1 T_k = T_k * (k - i) / (N - i);
 *            T_{n+1} = T_n * (n + 1) / (n + 1 - k); T'_k = 1, T'_{n+1} = T'_n +
 *            ceil(T_{n+1} - T_n).  The paper fixes T_N at 200 000 draws; here
 *            T_N is the call's own `iterations`, so the schedule reaches the
 *            whole set as the call ends (a pair of ten matches is not sampled
 *            from its top five a thousand times).
 *   Sample   n_h is the smallest n in [k, N] with h < T'_n: k - 1 distinct
 *            draws of the uniform calls' scheme below n_h - 1, then rank
 *            n_h - 1 as the last member.  Without such an n (h >= T'_N, reached
 *            when N is close to k) the uniform calls' k draws below N, over
 *            the ranked matches.  The hash is the uniform calls'.
 * Validity, solve, score, ties, "no model" and the refit rounds are the
 * uniform calls' on the ranked matches; best_hypothesis is the hypothesis
 * index, and inliers is in the caller's match order.  The params and result
 * structs, the other arguments, the checks and the guarantees are those of the
 * uniform siblings; the calls neither need nor change the call-sequence state.
 * SIFT_MI_EINVAL in addition, on the host before any device work: a quality
 * (or, with quality null, a match distance) that is NaN or infinite, or that
 * has its sign bit set (-0.0 included).
 * Limits: PROSAC's own stopping criteria are not built, because all hypotheses
 * of a call run at once.  The ranking counts, per match, the pair's smaller
 * keys: its cost is the sum over the pairs of N^2 compares, correct for every N
 * the uniform calls accept and quadratic in it; a sort is the remedy for pairs
 * of several 10^4 matches. */
int sift_mi_verify_pairs_progressive_device(sift_mi_ctx* ctx, const sift_mi_keypoint* d_kps, const size_t* offsets,
                                            uint32_t n_segs, const sift_mi_seg_pair* pairs, uint32_t n_pairs,
                                            const sift_mi_match* matches, const size_t* pair_offsets,
                                            const float* quality /* may be null: matches[i].distance */,
                                            const sift_mi_ransac_params* params,
                                            sift_mi_homography* models /* [n_pairs] */,
                                            uint8_t* inliers /* [pair_offsets[n_pairs]] */);
int sift_mi_verify_matches_progressive(sift_mi_ctx* ctx, const sift_mi_keypoint* query_kps, size_t n_query,
                                       const sift_mi_keypoint* train_kps, size_t n_train,
                                       const sift_mi_match* matches, size_t n_matches,
                                       const float* quality /* may be null: matches[i].distance */,
                                       const sift_mi_ransac_params* params, sift_mi_homography* model,
                                       uint8_t* inliers);
int sift_mi_verify_pairs_epipolar_progressive_device(sift_mi_ctx* ctx, const sift_mi_keypoint* d_kps,
                                                     const size_t* offsets, uint32_t n_segs,
                                                     const sift_mi_seg_pair* pairs, uint32_t n_pairs,
                                                     const sift_mi_match* matches, const size_t* pair_offsets,
                                                     const float* quality /* may be null: matches[i].distance */,
                                                     const sift_mi_ransac_params* params,
                                                     sift_mi_fundamental* models /* [n_pairs] */,
                                                     uint8_t* inliers /* [pair_offsets[n_pairs]] */);
int sift_mi_verify_matches_epipolar_progressive(sift_mi_ctx* ctx, const sift_mi_keypoint* query_kps, size_t n_query,
                                                const sift_mi_keypoint* train_kps, size_t n_train,
                                                const sift_mi_match* matches, size_t n_matches,
                                                const float* quality /* may be null: matches[i].distance */,
                                                const sift_mi_ransac_params* params, sift_mi_fundamental* model,
                                                uint8_t* inliers);

/* LABELLED EXTENSION (the step after the verification): guided matching.  The
 * pairs are matched again like sift_mi_match_pairs_device, but a query
 * keypoint competes only for the train keypoints the pair's model admits.
 * Element (i, j) of a pair is admissible when the verification's own inlier
 * test -- the same f32 operations in the same order -- holds for the record
 * (x_i, y_i, X_j, Y_j) under the pair's model and `threshold`:
 * SIFT_MI_MODEL_HOMOGRAPHY the test of sift_mi_verify_pairs_device (threshold
 * in px of the train image, and the query must lie in front of the
 * homography's horizon), SIFT_MI_MODEL_FUNDAMENTAL the Sampson test of
 * sift_mi_verify_pairs_epipolar_device (threshold = Sampson distance in px).
 * Nearest / second nearest (lowest (integer L2^2, index)), the distance and
 * the cross check are the unguided matcher's over the admissible elements
 * only: with cross_check, query i is kept only if its nearest admissible
 * train row's nearest admissible query is i.  The rule is stated in
 * tests/guided_ref.py and the result equals it bit for bit.
 *   ratio         > 0: kept only if distance[0] < ratio * distance[1] (f32,
 *                 one multiply, strict).  A query with exactly ONE admissible
 *                 candidate has no second neighbour, distance[1] = +inf, and
 *                 PASSES -- unlike sift_mi_match_ratio, which rejects a query
 *                 without a second neighbour: under a 3 px homography gate
 *                 most true matches have a single candidate.
 *   max_distance  > 0: kept only if distance[0] <= max_distance (the guard for
 *                 a lone candidate with an unrelated descriptor); 0: no cap.
 * A query with no admissible candidate has no match, and a pair whose model
 * is nine zeros (what the verification writes for "no model") gets an empty
 * range: a result, not an error.  With cross_check, ratio 0, no cap and the
 * verification's own model and threshold, every inlier of a verified
 * cross-checked match set is in the guided result.
 * Limits inherited from the verification: a scene that is one plane satisfies
 * a family of F, so under SIFT_MI_MODEL_FUNDAMENTAL the gate there is only as
 * good as the F that happened to win (use the homography); and an F gate
 * admits the whole band around an epipolar line, far more candidates than an
 * H gate's disc, so ratio and max_distance matter more with it.
 * models: n_pairs * 9 host f32, row-major, as sift_mi_homography.h /
 * sift_mi_fundamental.f.  d_desc, d_kps, offsets, pairs, out, cap,
 * pair_offsets: as sift_mi_match_pairs_device and sift_mi_verify_pairs_device
 * use them (segment-relative indices, query order, pair after pair; if cap is
 * too small, SIFT_MI_EINVAL with pair_offsets[n_pairs] set to the needed
 * count).  SIFT_MI_EINVAL, checked on the host before any device work: a
 * null argument, an unknown model_kind, a threshold that is not finite or
 * <= 0, a bad ratio (as sift_mi_match_ratio), a negative or NaN max_distance,
 * a model entry that is not finite, a pair index >= n_segs, decreasing
 * offsets.  The call only reads d_desc and d_kps and never invalidates the
 * device results; no allocation once the context's scratch has grown to the
 * call's size; its kernel time is added to sift_mi_stats.match_ms. */
typedef enum { SIFT_MI_MODEL_HOMOGRAPHY = 0, SIFT_MI_MODEL_FUNDAMENTAL = 1 } sift_mi_model_kind;
typedef struct {
    float threshold, ratio, max_distance;
    int cross_check;
} sift_mi_guided_params;
int sift_mi_match_pairs_guided_device(sift_mi_ctx* ctx, const uint8_t* d_desc, const sift_mi_keypoint* d_kps,
                                      const size_t* offsets, uint32_t n_segs, const sift_mi_seg_pair* pairs,
                                      uint32_t n_pairs, int model_kind, const float* models /* n_pairs * 9 */,
                                      const sift_mi_guided_params* params, sift_mi_match* out, size_t cap,
                                      size_t* pair_offsets);
/* The one-pair form on host descriptors and host keypoints: uploads them and
 * runs the same kernels; *n_matches as sift_mi_match_ratio sets it. */
int sift_mi_match_guided(sift_mi_ctx* ctx, const uint8_t* query, const sift_mi_keypoint* query_kps, size_t n_query,
                         const uint8_t* train, const sift_mi_keypoint* train_kps, size_t n_train, int model_kind,
                         const float* model /* 9 */, const sift_mi_guided_params* params, sift_mi_match* out,
                         size_t cap, size_t* n_matches);
/* Diagnostic: the 128 x 128 tiles the guided calls covered and the waves (four
 * per tile) that left at the cull (SIFT_MI_PATH_GUIDED_CULL); cumulative,
 * reset by sift_mi_reset_stats. */
int sift_mi_guided_counters(sift_mi_ctx* ctx, uint64_t* tiles, uint64_t* culled_waves);

/* ---- feature tracks (LABELLED EXTENSION: the crate has nothing like it) ----
 * Links the kept matches of the pairs into tracks: the connected components
 * of the graph whose nodes are the arena rows [offsets[0], offsets[n_segs])
 * and whose edges join row offsets[query_seg] + query_idx to row
 * offsets[train_seg] + train_idx for every match m of pair p, m in
 * [pair_offsets[p], pair_offsets[p + 1]), with keep[m] != 0 (keep null: every
 * match; the verification's inlier mask goes in unchanged).  The rule is
 * tests/tracks_ref.py's; every output is integer-exact.  A component's label
 * is its smallest row; it is in conflict when two of its rows lie in one
 * segment; it is a track when it has at least min_length (>= 2) rows and,
 * with drop_conflicts != 0, is not in conflict.  Tracks are numbered by
 * ascending label, a track's members listed by ascending row.
 *
 * Outputs, host arrays sized from N = offsets[n_segs] - offsets[0]:
 *   track_of[N]                    track of row offsets[0] + i, or -1
 *   *n_tracks, track_offsets[n_tracks + 1]   (N / 2 + 2 entries provided)
 *   obs[track_offsets[n_tracks]]   one record per member: its segment, its
 *                                  index in the segment, and the x, y bit
 *                                  patterns of its keypoint (N entries provided)
 *   conflict[n_tracks]             1 where the track is in conflict; all 0
 *                                  with drop_conflicts (N / 2 + 1 provided)
 * SIFT_MI_EINVAL, before any device work, for a null argument other than
 * keep, min_length < 2, a pair naming a segment >= n_segs, decreasing offsets
 * or pair_offsets, a match index outside its pair's segment, N or the match
 * count above 2^31 - 1, a d_kps that is not 4-byte aligned.  No pairs, no matches and N == 0 give no tracks.
 * Only reads d_kps: the device results stay valid; no allocation once the
 * context's scratch has grown to the call's size. */
typedef struct {
    uint32_t min_length;
    int drop_conflicts;
} sift_mi_track_params;
typedef struct {
    uint32_t seg, idx;
    float x, y;
} sift_mi_track_obs;
int sift_mi_build_tracks_device(sift_mi_ctx* ctx, const sift_mi_keypoint* d_kps, const size_t* offsets,
                                uint32_t n_segs, const sift_mi_seg_pair* pairs, uint32_t n_pairs,
                                const sift_mi_match* matches, const size_t* pair_offsets,
                                const uint8_t* keep /* may be null */, const sift_mi_track_params* params,
                                int32_t* track_of, uint32_t* n_tracks, uint32_t* track_offsets,
                                sift_mi_track_obs* obs, uint8_t* conflict);
/* Diagnostic: the kernel time of the track calls (two events around the
 * launch sequence) and the edges (kept matches) they linked; cumulative,
 * reset by sift_mi_reset_stats. */
int sift_mi_track_counters(sift_mi_ctx* ctx, double* kernel_ms, uint64_t* edges);

/* ---- frame-pair proposal (LABELLED EXTENSION: the crate has nothing like it) -
 * Which frames of an unordered batch to hand to sift_mi_match_pairs_device:
 * preemptive matching (C. Wu, "Towards linear-time incremental structure from
 * motion", 2013) of each segment's largest-scale features, on the arena
 * d_desc / d_kps / offsets[n_segs + 1] that the match and track calls take.
 * The rule is tests/pairs_ref.py's; every output is integer-exact.
 *   Subset   S_f = the min(rows of f, subset) rows of segment f with the
 *            largest keypoint `size`, compared as the u32 pattern of the f32
 *            (numeric order for the non-negative finite sizes SIFT emits),
 *            the lower row first among equals; kept in ascending row order.
 *   Score    scores[a * n_segs + b], a != b = the matches that
 *            sift_mi_match_ratio(S_a, S_b, ratio, cross_check = 1) keeps
 *            (ratio == 0: no ratio test; a query without a second neighbour
 *            fails a ratio test); 0 on the diagonal.  Symmetric when ratio
 *            == 0, not in general otherwise.
 *   Proposal s(a, b) = max(scores[a][b], scores[b][a]); a < b is a candidate
 *            when s >= min_matches.  max_partners == 0: every candidate is
 *            proposed.  Otherwise each frame keeps its first max_partners
 *            candidates by (s descending, partner ascending), and a pair is
 *            proposed when either of its two frames keeps it.
 * pairs[cap] receives the proposed (a, b), a < b, sorted by (a, b), *n_pairs
 * their number; scores (n_segs * n_segs, row-major) may be null.  One
 * workgroup per unordered pair computes both directions; only the scores come
 * back from the device.
 * Limits: subset <= 128 by construction (one 128 x 128 tile is a whole frame
 * pair); frames whose overlap holds few large-scale features score low and
 * are missed; min_matches is a setting to be chosen for the content, not a
 * law (DESIGN.md 3.16 has the figures behind the Python default of 8).
 * SIFT_MI_EINVAL, before any device work, for a null argument other than
 * scores, subset outside 1..128, a ratio outside [0, 1] or NaN, min_matches
 * == 0, decreasing offsets, n_segs > 4096 (a 64 MB score matrix), rows
 * above 2^31 - 1, a d_desc that is not 16-byte or a d_kps that is not 4-byte
 * aligned; and, after the run, for cap < *n_pairs (then *n_pairs is the
 * number needed and scores, if given, are written).  n_segs of 0 or 1 gives
 * no pairs.  Only reads d_desc and d_kps; no allocation once the context's
 * scratch has grown to the call's size. */
typedef struct {
    uint32_t subset;
    float ratio;
    uint32_t min_matches;
    uint32_t max_partners;
} sift_mi_pair_params;
int sift_mi_propose_pairs_device(sift_mi_ctx* ctx, const uint8_t* d_desc, const sift_mi_keypoint* d_kps,
                                 const size_t* offsets, uint32_t n_segs, const sift_mi_pair_params* params,
                                 uint32_t* scores /* n_segs * n_segs, may be null */, sift_mi_seg_pair* pairs,
                                 size_t cap, size_t* n_pairs);
/* Diagnostic: the kernel time of the proposal calls (two events around the
 * launch sequence) and the frame-pair tiles they computed, n_segs (n_segs -
 * 1) / 2 a call; cumulative, reset by sift_mi_reset_stats. */
int sift_mi_pair_counters(sift_mi_ctx* ctx, double* kernel_ms, uint64_t* tiles);

/* ---- spread-limited keypoints (LABELLED EXTENSION: the crate has nothing like it)
 * Adaptive non-maximal suppression (Brown, Szeliski, Winder, "Multi-image
 * matching using multi-scale oriented patches", 2005) on the arena d_kps /
 * d_desc / offsets[n_segs + 1] that the match and track calls take: up to
 * `limit` keypoints per segment, spread over the frame, where features_limit
 * keeps the strongest responses wherever they cluster.  The rule is
 * tests/select_ref.py's; every output equals it bit for bit.  Segments are
 * independent.  Within one, for row i (responses and positions as f32):
 *   Suppressor  row j suppresses row i when r_i < c * r_j: one f32 multiply,
 *               a strict comparison, 0 < c <= 1 (c == 1: only strictly
 *               stronger rows).  Rows of equal response never suppress each
 *               other, and a row never suppresses itself.
 *   Radius      R2_i = the minimum over its suppressors of
 *               (x_j - x_i) * (x_j - x_i) + (y_j - y_i) * (y_j - y_i), every
 *               operation a separately rounded f32 operation (no fused
 *               multiply-add); +inf without a suppressor.
 *   Selection   the min(rows, limit) rows with the largest R2, compared as the
 *               u32 pattern of the f32, the lower row first among equals;
 *               kept in ascending row order.
 * sel_offsets[n_segs + 1] receives the kept rows' segment bounds, rows[cap]
 * the kept rows, each relative to its segment's first row (what maps a match
 * on the compact arena back to the original keypoint), radius2 (may be null)
 * R2 of every row from offsets[0] to offsets[n_segs].  The kept keypoints and,
 * when d_desc is not null, their descriptors are gathered into a compact arena
 * in device memory in the same layout (sift_mi_selected_results): with
 * sel_offsets it goes straight into sift_mi_match_pairs_device,
 * sift_mi_verify_pairs_device, sift_mi_match_pairs_guided_device,
 * sift_mi_build_tracks_device and sift_mi_propose_pairs_device.
 * Inputs are assumed finite with responses >= 0, which holds for what the
 * extraction emits.  With a NaN, an infinity or a negative response in a
 * keypoint the call stays memory-safe and deterministic; its result is
 * otherwise unspecified.
 * Limits: the distance is 2-D position only, so keypoints of different scales
 * at one place compete; the keypoints SIFT emits per orientation peak at one
 * place have equal radii and are kept or cut by row order; `limit` is one
 * number for all segments.
 * SIFT_MI_EINVAL, before any device work, for a null argument other than
 * d_desc / radius2, limit == 0, c NaN or outside (0, 1], decreasing offsets,
 * rows above 2^31 - 1, a d_kps that is not 4-byte or a d_desc that is not
 * 16-byte aligned; and for cap < the rows kept (then sel_offsets is written
 * and sel_offsets[n_segs] is the number needed).  Empty segments give empty
 * ranges, n_segs == 0 nothing.  Only reads d_kps and d_desc (the extraction's
 * device results stay valid); no allocation once the context's scratch has
 * grown to the call's size. */
typedef struct {
    uint32_t limit;
    float c;
} sift_mi_select_params;
int sift_mi_select_spread_device(sift_mi_ctx* ctx, const sift_mi_keypoint* d_kps,
                                 const uint8_t* d_desc /* may be null */, const size_t* offsets, uint32_t n_segs,
                                 const sift_mi_select_params* params, size_t* sel_offsets /* n_segs + 1 */,
                                 uint32_t* rows, size_t cap, float* radius2 /* may be null */);
/* The compact arena of the last select call: *n kept keypoints and their
 * descriptors (*d_sel_desc null when that call had none) in device memory,
 * valid until the next select call or sift_mi_destroy.  n == 0 before any. */
int sift_mi_selected_results(sift_mi_ctx* ctx, const sift_mi_keypoint** d_sel_kps, const uint8_t** d_sel_desc,
                             size_t* n);
/* The one-frame host form: kps[n] in host memory, one segment, no
 * descriptors.  rows[cap] receives the kept rows, *n_rows = min(n, limit)
 * (the number needed when cap is smaller: SIFT_MI_EINVAL), radius2[n] may be
 * null. */
int sift_mi_select_keypoints(sift_mi_ctx* ctx, const sift_mi_keypoint* kps, size_t n,
                             const sift_mi_select_params* params, uint32_t* rows, size_t cap, size_t* n_rows,
                             float* radius2 /* may be null */);
/* Diagnostic: the kernel time of the select calls (two events around the
 * launch sequence) and the (row, candidate) pair tests they made, the sum of
 * rows^2 over a call's segments; cumulative, reset by sift_mi_reset_stats. */
int sift_mi_select_counters(sift_mi_ctx* ctx, double* kernel_ms, uint64_t* pair_tests);

/* ---- the input step before the path ---------------
 * Baseline (SOF0/SOF1) Huffman JPEG, 1 or 3 components -> 8-bit luma, with
 * the arithmetic of the reference's decode: image 0.25.2 `image::open` /
 * `load_from_memory` (zune-jpeg) then `.grayscale()` (examples/run-sift.rs:8,
 * src/lib.rs:1012).  Host entropy decoding, GPU IDCT / upsampling / colour.
 * sift_mi_jpeg_dims: frame size from the headers (host only, no device).
 * sift_mi_decode_jpeg: luma into out (row stride out_stride), a host buffer,
 * or device memory when out_on_device != 0 (ordered on the context stream;
 * the call returns once the frame is written).
 * Limits: the decode calls refuse a frame with a side above 16384 px (what
 * sift_mi_extract takes) with SIFT_MI_EINVAL, before anything is allocated
 * from the header; sift_mi_jpeg_dims still reports such a size.  Malformed
 * input is SIFT_MI_EINVAL, an unsupported frame (progressive, 12-bit, 4
 * components, sampling factors above 2, vertical-only chroma subsampling,
 * several scans) SIFT_MI_EUNSUPPORTED, a failed host or device allocation
 * SIFT_MI_ENOMEM; no C++ exception leaves these calls. */
int sift_mi_jpeg_dims(const uint8_t* data, size_t len, uint32_t* width, uint32_t* height);
int sift_mi_decode_jpeg(sift_mi_ctx* ctx, const uint8_t* data, size_t len, uint8_t* out, size_t out_stride,
                        int out_on_device);
/* n JPEGs of one size and sampling -> device luma frames laid out as
 * sift_mi_extract_batch_device takes them (frame i at d_frames + i *
 * frame_pitch, rows row_stride apart).  Entropy decoding runs on `threads`
 * host threads (<= 0: up to 16), overlapped with the GPU reconstruction of
 * the previous chunk of frames; returns once every frame is written. */
int sift_mi_decode_jpeg_batch(sift_mi_ctx* ctx, const uint8_t* const* data, const size_t* len, uint32_t n,
                              uint8_t* d_frames, size_t frame_pitch, size_t row_stride, int threads);

/* ---- measurement ---------------------------------------------------------
 * Cumulative since the last reset.  The stage times (pyramid_ms ..
 * descriptor_ms, total_ms) come from HIP events that only the one-lane mode
 * records (sift_mi_set_pipeline_lanes(ctx, 1): the stage-timing mode; a
 * marker costs ~7 us of a stream's timeline, so the two-lane throughput mode
 * records none and leaves them at 0).  pyramid_* covers the seed + octave
 * blur kernels (the HBM-bound stage), which include the extremum scan of the
 * octaves detected with their last blur (k_blur_detect); pyramid_bytes is
 * SURVEY.md 8(d)'s algorithmic byte count W*H + 44*sum(P_o) per frame, and
 * pyramid_scan_bytes what the reference's scan reads for those fused
 * octaves (the five DoG planes once, 20 B per octave pixel), apart. */
typedef struct {
    double pyramid_ms;
    double detect_ms;
    double orient_ms;
    double order_ms;
    double descriptor_ms;
    double total_ms;
    uint64_t pyramid_bytes;
    uint64_t pyramid_launches;
    uint64_t frames;
    uint64_t extrema;
    uint64_t keypoints;
    uint64_t band_reruns;  /* row-band calls re-run on the whole-frame pyramid (sift_mi_set_row_band) */
    uint64_t stage_reruns; /* chunks re-run because a stage count exceeded its buffer bound */
    /* gradient samples evaluated (sift_mi_set_sample_counting on, else 0):
     * orientation = patch positions of gradient_direction_histogram
     * (src/lib.rs:657-757) inside the image, descriptors = samples of the
     * rotated 4x4 region that compute_descriptor (src/lib.rs:785-990) enumerates */
    uint64_t orient_samples;
    uint64_t desc_samples;
    uint64_t pyramid_scan_bytes;
    /* the segmented matcher (sift_mi_match_pairs_device, sift_mi_match_ratio,
     * sift_mi_match_neighbors): its kernels' time from HIP events around them
     * (every call records the two), and the 128 x 128 tiles they covered */
    double match_ms;
    uint64_t match_tiles;
} sift_mi_stats;
int sift_mi_get_stats(sift_mi_ctx* ctx, sift_mi_stats* out);
int sift_mi_reset_stats(sift_mi_ctx* ctx);
/* Measurement only: count the samples the orientation and descriptor kernels
 * evaluate (one device atomic per workgroup / per descriptor wave; off by
 * default, and off in every timed run).  Read with sift_mi_get_stats. */
int sift_mi_set_sample_counting(sift_mi_ctx* ctx, int on);

/* Library version string and last error (thread-local).
 * 0.5.0: sift_mi_match_neighbors, sift_mi_match_ratio,
 *        sift_mi_match_pairs_device (2-NN, ratio test, segment pairs of a
 *        device arena); sift_mi_stats gained match_ms, match_tiles (a larger
 *        struct); sift_mi_device_results stay valid across match calls.
 *        Added later under the same version (no existing symbol or struct
 *        changed): sift_mi_verify_pairs_device, sift_mi_verify_matches
 *        (RANSAC homography + inlier refit of matched pairs);
 *        sift_mi_verify_pairs_epipolar_device, sift_mi_verify_matches_epipolar
 *        (RANSAC fundamental matrix + inlier refit; sift_mi_fundamental);
 *        sift_mi_match_pairs_guided_device, sift_mi_match_guided,
 *        sift_mi_guided_counters (guided matching under the verified models;
 *        sift_mi_model_kind, sift_mi_guided_params), SIFT_MI_PATH_GUIDED_CULL;
 *        sift_mi_build_tracks_device, sift_mi_track_counters (feature tracks
 *        over the kept matches; sift_mi_track_params, sift_mi_track_obs);
 *        sift_mi_propose_pairs_device, sift_mi_pair_counters (frame pairs
 *        proposed by preemptive matching; sift_mi_pair_params);
 *        sift_mi_select_spread_device, sift_mi_selected_results,
 *        sift_mi_select_keypoints, sift_mi_select_counters (spread-limited
 *        keypoints by adaptive non-maximal suppression; sift_mi_select_params);
 *        sift_mi_verify_pairs_progressive_device,
 *        sift_mi_verify_matches_progressive,
 *        sift_mi_verify_pairs_epipolar_progressive_device,
 *        sift_mi_verify_matches_epipolar_progressive (the two verifications
 *        with quality-ordered PROSAC samples; the uniform calls' structs).
 *        The call-sequence contract at the top of this file (no symbol
 *        changed): sift_mi_fetch / sift_mi_device_results answer for the call
 *        that produced the last result, not for the current keep_on_device
 *        setting; a refused or failed call leaves what the contract says.
 * 0.4.0: sift_mi_set_path_option (replaces the environment knobs),
 *        sift_mi_batch_octave_dims, sift_mi_read_batch_scale_space takes the
 *        output capacity, sift_mi_stats gained pyramid_scan_bytes (pyramid_bytes
 *        no longer includes it).
 * 0.3.0: no ABI change from 0.2.
 * 0.2.0: emission keys (sift_mi_fetch_keys) widened x / y to 15 bits -- image
 *        field moved from bit 40 to bit 42; sift_mi_stats gained band_reruns,
 *        stage_reruns, orient_samples, desc_samples (a larger struct). */
const char* sift_mi_version(void);
const char* sift_mi_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SIFT_MI_H */
