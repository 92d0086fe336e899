// Host-side launch interface of the HIP kernels (internal to libsift_mi.so).
#pragma once

#include <string>

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "sift_common.h"

namespace siftmi {

// cv::resize coefficient tables (device pointers), resizeGeneric_ layout.
struct ResizeTab {
    const int* xofs;
    const float* xa0;
    const float* xa1;
    const int* yofs;
    const float* ya0;
    const float* ya1;
    int xmax;
};

// image::imageops::resize sampling tables (ImageprocProcessing profile),
// per destination index: first source tap and up to kIpTaps normalised f32
// weights (zero-padded; an extra zero-weight tap adds +0 and changes nothing).
constexpr int kIpTaps = 3;
struct IpResizeTab {
    const int* xl;
    const float* xw;  // [dst_w][kIpTaps]
    const int* yl;
    const float* yw;  // [dst_h][kIpTaps]
};

// Arithmetic profile of the Processing backend (src/lib.rs:86-90).
enum : int { kProfileOpenCV = 0, kProfileImageproc = 1 };

// Kernel-path switches of one context (sift_mi_set_path_option).  The
// defaults are the product path; every alternative computes the same bits and
// exists so the tests can hold each kernel family against the oracle.  They
// live in the context (no process-wide state, nothing read from the
// environment).
// Onesweep from this many sort keys (PathOpts::onesweep = 2): below it rocprim's
// block sort + merge path is faster.  One 1080p frame (~12 k keys): 0.578 vs
// 0.71 ms per call with Onesweep; 256 x VGA (128-frame chunks, ~206 k keys):
// 10.08-10.29 vs 9.93-10.15 ms; 128 x 1080p (64-frame chunks, ~715 k keys):
// 31.69-31.73 vs 31.68-31.89 ms (profiles/r05_batch35.log, r05_vga35.log)
constexpr uint32_t kOnesweepMinKeys = 1u << 19;

struct PathOpts {
    int tile_blur = 0;     // 1: one-tile-per-workgroup blurs everywhere (no strip / pair kernels)
    int pair = 1;          // 0: no pair kernels (k_blur2_strip, k_seed_pair)
    int seed_pair = 1;     // 0: k_seed_strip, then blur 1 like the other octaves
    int tail = 1;          // 0: per-blur launches for the small octaves (no k_octave_tail)
    int fused_detect = 1;  // 0: blur 5 and the extremum scan apart; 2: fused at 32-row segments wherever it applies
    int early = 1;         // one-chunk calls: detection of the octaves below the tail beside the tail kernel
    int desc_first = 1;    // one-frame calls: descriptors beside the ordering stage
    int graph = 0;         // 1: single-chunk calls captured once and replayed as a HIP graph
    int band_drift = 24;   // row bands: refinement drift accepted without a re-run (< 24 forces re-runs)
    int bound_shrink = 1;  // > 1: first-chunk stage bounds divided by it (forces the overflow re-run)
    int large_first = 1;   // one-chunk early path: two-ended extremum append (RefineLaunch::counter_hi)
    int bd_pair = 1;       // 1: k_blur_detect_pair (two column strips per lane, packed f32); 0: the
                           // one-column k_blur_detect (2, once a 4-row loop form of the pair kernel, is read as 1)
    int bd_waves = 8192;   // k_blur_detect_pair: fewest waves per launch at the chosen row segments
    int chunk_mode = 1;    // automatic chunking (SIFT_MI_PATH_CHUNK_MODE)
    int guided_cull = 1;   // guided matcher: a wave whose 64 x 64 block admits nothing skips its loads and MFMAs
    int onesweep = 0;      // emission-order sorts with rocprim's Onesweep: 1 always, 0 never (the
                           // library default path), 2 for bounds >= kOnesweepMinKeys
};

// Image planes are row-pitched: element (y, x) at plane[y * pitch + x].
struct BlurLaunch {
    const float* src;
    size_t src_img_stride;
    float* dst;
    size_t dst_img_stride;
    float* nxt;  // may be null: next octave base (nearest 1/2)
    size_t nxt_img_stride;
    int pitch_n, wn, hn;
    int W, H, pitch;
    int n_img;
    int y0, y1;  // output rows [y0, y1) only (rounded out to tiles); y1 <= y0: all rows
    BlurTaps taps;
    int profile;  // kProfileOpenCV | kProfileImageproc
};

struct SeedLaunch {
    const uint8_t* frames;
    size_t frame_pitch, row_stride;
    int sh, sw;      // source height, width
    ResizeTab tab;   // 2x bilinear tables (OpenCV profile)
    IpResizeTab iptab;  // 2x Triangle tables (Imageproc profile)
    int profile;
    float* dst;      // octave 0, plane 0
    size_t dst_img_stride;
    int W, H, pitch;  // seed (2x) geometry
    int n_img;
    int y0, y1;  // output rows [y0, y1) only (rounded out to tiles); y1 <= y0: all rows
    BlurTaps taps;
    // k_seed_pair's first workgroup also resets a chunk's counters (k_chunk_init's
    // words: 4 zeros, init_m x ~0, init_words zeros) when init_cnt is set
    uint32_t* init_cnt = nullptr;
    int init_m = 0, init_words = 0;
};


// Host wait for an event (pipeline.cpp): spins ~1 ms, then polls with short
// sleeps, so a thread waiting for a multi-ms chunk does not hold a CPU the
// decode threads (or a CPU quota) need.
hipError_t host_wait_event(hipEvent_t e);

// jpeg.hip: baseline JPEG -> 8-bit luma (zune-jpeg + image::grayscale arithmetic)
int jpeg_dims(const uint8_t* data, size_t len, uint32_t* w, uint32_t* h, std::string& err);
int jpeg_decode_luma(const uint8_t* data, size_t len, uint8_t* out, size_t out_stride, bool out_on_device,
                     hipStream_t st, std::string& err);
// pinned coefficient buffers and device scratch of the batch decoder, kept by
// the context across calls (grow-only)
struct JpegBatchCache {
    int16_t* pin[2] = {nullptr, nullptr};
    hipEvent_t up[2] = {nullptr, nullptr};
    size_t pin_bytes = 0;
    uint8_t* dev = nullptr;
    size_t dev_bytes = 0;
    void release();
};
int jpeg_decode_batch(const uint8_t* const* data, const size_t* len, uint32_t n, uint8_t* d_out, size_t frame_pitch,
                      size_t stride, int threads, hipStream_t st, JpegBatchCache& cache, std::string& err);

// Every octave from o0 on of n_img frames in one launch (k_octave_tail): a
// workgroup per frame, the octave's planes in LDS.  The octave G bases are
// the lane arena's; G_0 of octave o0 must be in place.
constexpr int kTailMaxOct = 16;
constexpr int kTailLdsFloats = 39680;  // 155 KB: A, B, T with halos + the next G_0 (pyramid.hip)
struct TailLaunch {
    float* gauss[kTailMaxOct];
    size_t gstride[kTailMaxOct];
    int ow[kTailMaxOct], oh[kTailMaxOct], pitch[kTailMaxOct];
    int o0, n_oct, n_img, profile;
    int r[kImagesPerOctave];
    BlurTaps taps[kImagesPerOctave];
};
// first octave that fits the tail kernel (n_oct: none); radii[1..5] = the
// octave's blur radii
int tail_octave_start(const int* ow, const int* oh, int n_oct, const int* radii);
void launch_octave_tail(const TailLaunch& L, hipStream_t st);

// pyramid.hip
// (a launcher's next kernel carries the completion event of a LaunchDoneEvent
// in scope: launch_ext.h)
int launch_blur(int radius, const BlurLaunch& L, hipStream_t st, const PathOpts& o = PathOpts{});
// two consecutive blurs of an octave (A then B, B.src == A.dst) in one pass;
// -1 when the pair kernel does not apply (the caller launches them singly)
int launch_blur_pair(int ra, int rb, const BlurLaunch& A, const BlurLaunch& B, hipStream_t st,
                     const PathOpts& o = PathOpts{});
int launch_seed(int radius, const SeedLaunch& L, hipStream_t st, const PathOpts& o = PathOpts{});
// the seed (radius rs) and blur 1 (radius rb; B.src == L.dst) in one pass
// (k_seed_pair: G_0 never read back); -1 when it does not apply
int launch_seed_pair(int rs, int rb, const SeedLaunch& L, const BlurLaunch& B, hipStream_t st,
                     const PathOpts& o = PathOpts{});
// D_s = G_{s+1} - G_s (s < 5) of an octave's G stack, for n images
void launch_dog(const float* gauss, size_t plane, size_t g_img_stride, float* dog, size_t dog_img_stride, int W, int H,
                int pitch, int n_img, hipStream_t st);
void launch_resize_linear_f32(const float* src, int sw, int sh, const ResizeTab& tab, float* dst, int dw, int dh,
                              hipStream_t st);
// image::imageops::resize (Imageproc profile, op level): generic tap tables
// with up to `taps` entries per index ([n][taps] weights)
void launch_ip_resize_f32(const float* src, int sw, int sh, const int* xl, const float* xw, int xtaps, const int* yl,
                          const float* yw, int ytaps, float* tmp, float* dst, int dw, int dh, hipStream_t st);
void launch_resize_nearest_f32(const float* src, int sw, const int* xofs, const int* yofs, float* dst, int dw, int dh,
                               hipStream_t st);

// detect.hip
// One launch over several octaves: octave i's strips take the blocks
// [block0[i], block0[i + 1]).
struct DetectOctave {
    const float* gauss;  // octave G_0 base, image b at gauss + b*img_stride, plane s at + s*pitch*H
    size_t img_stride;   // (the DoG planes are formed from G_0..G_5 as they are read)
    int W, H, pitch, octave;
    int y_lo, y_hi;  // candidate rows [y_lo, y_hi) (a row band; 0, H for the whole octave)
};
struct DetectLaunch {
    DetectOctave oct[kTailMaxOct];
    uint32_t block0[kTailMaxOct + 1];
    int n_oct, n_img, img_base;
    int sh;          // rows per strip (filled by launch_detect)
    uint64_t* cand;  // packed candidate keys (frame, octave, scale, y, x)
    uint32_t* counter;
    uint32_t cap;
};
// octaves L.oct[0 .. n_oct) (block0 and sh are filled here)
void launch_detect(DetectLaunch& L, hipStream_t st);
// The octave's blur 5 (G_4 -> G_5, radius R, whole planes) and its
// detection in one pass (k_blur_detect); -1 when it does not apply (the
// caller then runs launch_blur and the octave's k_detect_rows).  nsx, nsy,
// seg are filled here.
struct BlurDetectLaunch {
    float* gauss;       // octave G_0 base of the launch's first frame
    size_t img_stride;  // floats between frames
    int W, H, pitch, octave, n_img, img_base, profile;
    int nsx, nsy, seg;
    BlurTaps taps;      // blur 5
    uint64_t* cand;
    uint32_t* counter;
    uint32_t cap;
};
int launch_blur_detect(int R, BlurDetectLaunch& L, hipStream_t st, const PathOpts& o = PathOpts{});
// whether launch_blur_detect would launch (the same test, nothing enqueued)
bool blur_detect_applies(int R, const BlurDetectLaunch& L, const PathOpts& o = PathOpts{});

// Device tables of one lane's pyramid, indexed by octave: what the keypoint
// stages need to address any Gaussian of any frame of the chunk.
struct OctaveView {
    const float* const* gauss;  // octave G_0 bases (the DoG is formed from G_0..G_5 where it is read)
    const size_t* img_stride;   // floats between frames
    const int* ow;
    const int* oh;
    const int* opitch;
};

// Stage sizes live in device counters (no host round trip between stages):
// every consumer reads its count from device memory, clamps it to the buffer
// bound, and walks the items with a grid-stride loop.
struct RefineLaunch {
    const uint64_t* cand;
    const uint32_t* n_cand;  // device count (may exceed cand_cap: overflow, clamped)
    uint32_t cand_cap;
    // row bands with a restricted pyramid (null flag: no check): octave o's
    // Gaussians are exact on rows [H_o*r/n - 1 - margin, H_o*(r+1)/n + 1 + margin)
    // (clipped); the flag is set when a refinement reads outside them or an
    // accepted keypoint's patch (+-patch rows) leaves them
    uint32_t* band_flag;
    int band_r, band_n, band_margin, band_patch;
    OctaveView oct;
    int n_oct;  // entries of oct's device arrays
    int img_base;
    ExtRec* out;
    uint32_t* counter;
    uint32_t cap;
    // two-ended append (null: off): extrema whose windows will be large
    // (refined scale s + off_s >= kLargeWindowScale) from the front
    // (counter), the others from the back (out[cap - 1 - j], j from
    // counter_hi), so k_orient takes the large windows first (longest-first
    // scheduling of one frame's orientation: 0.574-0.576 vs 0.580-0.581 ms
    // per 1080p call; the descriptor kernel's duration did not change, its
    // keypoints are appended in orientation completion order)
    uint32_t* counter_hi;
};
constexpr float kLargeWindowScale = 2.0f;
void launch_refine(const RefineLaunch& L, hipStream_t st);

struct OrientLaunch {
    const ExtRec* ext;
    const uint32_t* n_ext;  // device count, clamped to ext_cap
    const uint32_t* n_ext_hi;  // two-ended ext (RefineLaunch::counter_hi; null: off): back-end count
    uint32_t ext_cap;
    OctaveView oct;
    KpRec* out;
    uint32_t* counter;
    int img_base;
    uint32_t cap;
    unsigned long long* samples;  // 8 counters (measurement only; null: off)
};
void launch_orient(const OrientLaunch& L, hipStream_t st);

// order.hip
// keys/vals for the emission-order sort; returns temp bytes when temp == null.
size_t sort_pairs_u64(void* temp, size_t temp_bytes, const uint64_t* kin, uint64_t* kout, const uint32_t* vin,
                      uint32_t* vout, uint32_t n, int end_bit, hipStream_t st,
                      bool onesweep = false);
// keys[i] = emission key of kp i for i < min(*n, bound); keys beyond are
// padded with `pad` (sorts last); vals[i] = i
void launch_chunk_init(uint32_t* cnt, int m, int work_words, hipStream_t st);
void launch_make_sort_keys(const KpRec* kp, const uint32_t* n, uint32_t bound, uint64_t pad, uint64_t* keys,
                           uint32_t* vals, hipStream_t st);
// starts[f] = first index of frame f in the sorted keys (0xffffffff if none);
// starts must be pre-filled with 0xff bytes
void launch_frame_starts(const uint64_t* sorted_keys, const uint32_t* n, uint32_t bound, uint32_t* starts,
                         hipStream_t st);
// Per-frame output plan (features_limit, src/lib.rs:156-161), one wave:
// out_cnt[f], seg_off[f] (first sorted index of frame f), out_off[f] (first
// output index), use_resp[f] (frame truncated by response) and *n_out.
void launch_limit_plan(const uint32_t* starts, const uint32_t* n_kp, uint32_t bound, int n_img, int64_t limit,
                       uint32_t* out_cnt, uint32_t* seg_off, uint32_t* out_off, uint8_t* use_resp, uint32_t* n_out,
                       hipStream_t st);
// key = (frame << 32) | ~bits(response) over the emission order; padded beyond *n
void launch_make_resp_keys(const KpRec* kp, const uint32_t* order, const uint32_t* n, uint32_t bound, int img_base,
                           uint64_t pad, uint64_t* keys, uint32_t* vals, hipStream_t st);
// final[i] = src index for i < *n_out: for frame f, if use_resp[f] the
// response order, else the emission order
// one-frame calls: descriptors computed in keypoint index order (desc_in),
// then row j of the outputs = keypoint order[j] (descriptor, KeyPoint, key)
void launch_gather_out(const KpRec* kp, const uint32_t* order, const uint32_t* n_out, uint32_t bound,
                       const uint8_t* desc_in, uint8_t* desc_out, OutKp* out_kp, uint64_t* out_key, uint64_t key_base,
                       const uint32_t* cnt, uint32_t* h_cnt, int cnt_words, hipStream_t st);
void launch_select(const uint32_t* emis_order, const uint32_t* resp_order, const uint32_t* seg_off,
                   const uint32_t* out_off, const uint8_t* use_resp, int n_img, const uint32_t* n_out, uint32_t bound,
                   uint32_t* final_idx, hipStream_t st);

// match.hip: per query the nearest train row (or -1), its distance
void launch_match(const uint8_t* q, int nq, const uint8_t* t, int nt, int cross_check, float* qn, float* tn,
                  unsigned long long* row_best, unsigned long long* col_best, int* train_idx, float* dist,
                  hipStream_t st);

// Segmented 2-NN matching of (query segment, train segment) pairs of one
// descriptor arena.  pairs[n_pairs + 1] (the last entry closes the prefixes):
// the segments' first arena rows and lengths, the pair's first slot in the
// per-(pair, query) arrays (best / second / outputs) and in the per-(pair,
// train) col_best, and its first 128 x 128 tile of the 1-D grid.
struct MatchPair {
    uint32_t qrow0, nq, trow0, nt, qoff, toff, tile0, pad;
};
// norm_blocks[b] = (first arena row, rows <= 256) of the segments in use; nrm
// is indexed by arena row.  nb_idx / nb_dist (2 per slot) may be null.
// ratio == 0: no ratio test.
void launch_match_pairs(const uint8_t* d, const MatchPair* pairs, int n_pairs, uint32_t n_tiles, uint32_t n_slots,
                        uint32_t n_cols, const uint2* norm_blocks, uint32_t n_norm_blocks, int cross_check,
                        float ratio, int* nrm, unsigned long long* best, unsigned long long* second,
                        unsigned long long* col_best, int* train_idx, float* dist, int* nb_idx, float* nb_dist,
                        hipStream_t st);
// The steps around its tile kernel, shared with the guided matcher: the
// memsets of best / second / col_best and the norms, and the final pass
// (max_distance == 0 and lone_passes == 0: the unguided rule; k_match_seg_final).
void launch_match_seg_prepare(const uint8_t* d, uint32_t n_slots, uint32_t n_cols, const uint2* norm_blocks,
                              uint32_t n_norm_blocks, int* nrm, unsigned long long* best, unsigned long long* second,
                              unsigned long long* col_best, hipStream_t st);
void launch_match_seg_final(const MatchPair* pairs, int n_pairs, uint32_t n_slots, const unsigned long long* best,
                            const unsigned long long* second, const unsigned long long* col_best, int cross_check,
                            float ratio, float max_distance, int lone_passes, int* train_idx, float* dist, int* nb_idx,
                            float* nb_dist, hipStream_t st);

// match_guided.hip
// launch_match_pairs over the elements the pairs' models admit (LABELLED
// EXTENSION; tests/guided_ref.py is the definition).  kps: the keypoints of the
// arena's rows; models[n_pairs * 9]: H or F per pair (device memory); qterm
// [n_slots], tterm[n_cols], culled[n_tiles] are scratch; *n_culled receives
// the waves that left at the cull (cull != 0).
void launch_match_pairs_guided(const uint8_t* d, const OutKp* kps, const MatchPair* pairs, int n_pairs,
                               uint32_t n_tiles, uint32_t n_slots, uint32_t n_cols, const uint2* norm_blocks,
                               uint32_t n_norm_blocks, bool fundamental, const float* models, float thr, int cull,
                               int cross_check, float ratio, float max_distance, int* nrm, unsigned long long* best,
                               unsigned long long* second, unsigned long long* col_best, float4* qterm, float4* tterm,
                               uint32_t* culled, unsigned long long* n_culled, int* train_idx, float* dist,
                               hipStream_t st);

// verify.hip
// RANSAC homography + inlier refit of matched pairs (LABELLED EXTENSION;
// tests/verify_ref.py is the definition).  pairs[n_pairs]: the pair's first
// record / match and its match count, and the first keypoint rows of its two
// segments.  VerifyMatch / VerifyModel are sift_mi_match / sift_mi_homography.
struct VerifyPair {
    uint32_t rec0, m, qrow0, trow0;
};
struct VerifyMatch {
    int32_t query_idx, train_idx;
    float distance;
};
struct VerifyModel {
    float h[9];
    uint32_t n_matches, n_inliers;
    int32_t best_hypothesis;
    uint32_t refits;
};
constexpr int kVerifyChunk = 1024;  // records of a pair in LDS at a time (k_verify_score)
// Progressive (PROSAC) sampling (LABELLED EXTENSION; tests/prosac_ref.py is the
// definition): the records are gathered in rank order and each
// hypothesis draws from the best n_h of them.  Null where a launch takes one:
// uniform sampling, the kernels and results of before.
constexpr int kVerifyRankRows = 512;    // matches of a pair per workgroup of k_verify_gather_ranked
constexpr int kVerifyRankStage = 1024;  // keys of a pair in LDS at a time
struct VerifyProgressive {
    const float* quality;    // [n_rec] finite, sign bit clear (the host checked); null: matches[i].distance
    const uint32_t* growth;  // [n_rec] per pair its slice of the growth table (prosac_growth.h)
    const uint2* wgs;        // [n_wgs] (pair, first match of the workgroup within it), kVerifyRankRows apart
    uint32_t n_wgs;
    uint32_t* perm;          // [n_rec] scratch: the caller's match (within its pair) at each rank
};
// matches[n_rec] hold indices the host has checked against their segments.
// rec[n_rec], models[n_pairs * iterations * 9], best[n_pairs] are scratch;
// out[n_pairs] and inliers[n_rec] the results.
void launch_verify(const OutKp* kps, const VerifyMatch* matches, const VerifyPair* pairs, int n_pairs, uint32_t n_rec,
                   float thr, uint32_t iterations, uint32_t seed, uint32_t refit_rounds, float4* rec, float* models,
                   unsigned long long* best, VerifyModel* out, uint8_t* inliers, hipStream_t st,
                   const VerifyProgressive* prog = nullptr);

void launch_verify_gather(const OutKp* kps, const VerifyMatch* matches, const VerifyPair* pairs, int n_pairs,
                          uint32_t n_rec, float4* rec, hipStream_t st);
// rec and prog.perm in rank order; the cost is the sum of m^2 key compares over the pairs
void launch_verify_gather_ranked(const OutKp* kps, const VerifyMatch* matches, const VerifyPair* pairs,
                                 const VerifyProgressive& prog, float4* rec, hipStream_t st);

// verify_epipolar.hip
// RANSAC fundamental matrix + eigen-refit of matched pairs (LABELLED
// EXTENSION; tests/epipolar_ref.py is the definition).  The arguments are
// launch_verify's, plus box[n_pairs * 6] (scratch: the f64 box normalisation
// of each pair); VerifyModel is sift_mi_fundamental as well (h holds F).
void launch_verify_epipolar(const OutKp* kps, const VerifyMatch* matches, const VerifyPair* pairs, int n_pairs,
                            uint32_t n_rec, float thr, uint32_t iterations, uint32_t seed, uint32_t refit_rounds,
                            float4* rec, double* box, float* models, unsigned long long* best, VerifyModel* out,
                            uint8_t* inliers, hipStream_t st, const VerifyProgressive* prog = nullptr);

// tracks.hip
// Feature tracks: connected components of the kept matches over the arena's
// rows (LABELLED EXTENSION; tests/tracks_ref.py is the definition).  Rows are
// relative to the call's first row; pair p's matches are [rec0, next pair's
// rec0), its segments start at rows qrow0 / trow0.  TrackObs is
// sift_mi_track_obs.
struct TrackPair {
    uint32_t rec0, qrow0, trow0;
};
struct TrackObs {
    uint32_t seg, idx;
    float x, y;
};
constexpr uint32_t kTrackLdsSegs = 2048;  // segment starts k_track_init searches in LDS (more: in global memory)
struct TrackLaunch {
    const OutKp* kps;            // the call's first row
    const uint32_t* offs;        // [n_segs] first row of each segment (offs[0] = 0)
    uint32_t n_segs, n_rows;
    const VerifyMatch* matches;  // [n_matches] indices the host has checked against their segments
    const uint8_t* keep;         // [n_matches] or null: all kept
    const TrackPair* pairs;      // [n_pairs], rec0 ascending from 0
    uint32_t n_pairs, n_matches;
    uint32_t min_length;
    int drop_conflicts;
    // scratch, n_rows entries each unless noted
    uint32_t *parent, *seg_of, *label, *row, *sorted_label, *sorted_row, *start, *end;
    uint8_t* confl;
    uint2* bsum;                 // ceil(n_rows / 256)
    void* sort_temp;
    size_t sort_temp_bytes;      // track_sort_temp_bytes(n_rows)
    // results
    uint32_t* totals;            // tracks, members
    int32_t* track_of;           // [n_rows]
    uint32_t* track_offsets;     // [n_rows / 2 + 2]
    TrackObs* obs;               // [n_rows]
    uint8_t* conflict;           // [n_rows / 2 + 1]
};
size_t track_sort_temp_bytes(uint32_t n_rows);  // 0: the query failed
// The launch sequence on st (nothing with n_rows == 0); -1 when the sort could not be enqueued.
int launch_tracks(const TrackLaunch& L, hipStream_t st);

// pairs.hip
// Frame-pair proposal by preemptive matching (LABELLED EXTENSION;
// tests/pairs_ref.py is the definition).  kps / d: the call's first row;
// offs[n_segs + 1]: the segments' first rows from it.  cnt[n_segs],
// sub_d[n_segs * h * 128] and sub_m[n_segs * h] are scratch (each segment's
// min(rows, h) largest-size rows, gathered); score[n_segs * n_segs] receives
// every entry: score[a][b] = kept matches of S_a -> S_b, 0 on the diagonal.
// 1 <= h <= kPairSubsetMax; ratio == 0: no ratio test.
constexpr uint32_t kPairSubsetMax = 128;  // one 128 x 128 tile is a whole frame pair
void launch_pairs(const OutKp* kps, const uint8_t* d, const uint32_t* offs, uint32_t n_segs, uint32_t h, float ratio,
                  uint32_t* cnt, uint8_t* sub_d, int* sub_m, uint32_t* score, hipStream_t st);

// select.hip
// Spread-limited selection by adaptive non-maximal suppression (LABELLED
// EXTENSION; tests/select_ref.py is the definition).  kps / d: the call's
// first row (d may be null: no descriptors); offs[n_segs + 1]: the segments'
// first rows from it; sel_offs[n_segs + 1]: the running sums of min(n_s,
// limit), total = their last; wgs[n_wgs] = (segment, first query row) of each
// radius workgroup, kSelectRowsPerWg rows apiece, none of them spanning two
// segments.  r2[rows of the arena], rows / src[total] and the compact arena
// sel_kps[total], sel_d[total * 128] (unused when d is null) are written.
constexpr uint32_t kSelectRowsPerWg = 512;
struct SelectLaunch {
    const OutKp* kps;
    const uint8_t* d;
    const uint32_t *offs, *sel_offs;
    const uint2* wgs;
    uint32_t n_segs, n_wgs, n_rows, total, limit;  // n_rows: the arena's rows, offs[n_segs]
    float c;
    float* r2;
    uint32_t *rows, *src;
    OutKp* sel_kps;
    uint8_t* sel_d;
};
void launch_select(const SelectLaunch& L, hipStream_t st);

// describe.hip
// Descriptor work queues: keypoint i belongs to queue i % kDescQueues, which
// hands out its keypoints in order; 8 counters on separate 128-B lines (one
// per XCD) keep the same-address atomic rate at an eighth.
constexpr int kDescQueues = 8;
constexpr int kDescQueueStride = 32;  // uint32 words
constexpr int kDescWorkWords = kDescQueues * kDescQueueStride;

struct DescLaunch {
    const KpRec* kp;
    const uint32_t* idx;  // final order -> kp index (may be null = identity)
    const uint32_t* n;    // device count, clamped to bound
    uint32_t bound;
    uint32_t* work;       // kDescQueues zeroed work counters, kDescQueueStride words apart: waves
                          // take keypoints dynamically (costs vary ~20x)
    uint64_t key_base;    // added to the emission keys (frame offset of the chunk)
    OctaveView oct;
    int img_base;
    OutKp* out_kp;     // may be null
    uint64_t* out_key; // may be null
    uint8_t* out_desc;
    int exact;         // 1: bit-exact bin-owner accumulation (describe_wave_exact)
    unsigned long long* samples;  // 8 counters (measurement only; null: off)
    // micro-benchmark probes (k_describe's kAblate bit 5 only; null in the product)
    float* probe_raw;                 // 128 bin sums per keypoint before normalisation
    unsigned long long* probe_iters;  // sample-loop iterations, four-round iterations
};
void launch_describe(const DescLaunch& L, hipStream_t st);

// single-keypoint compute_descriptor on an arbitrary f32 image
void launch_describe_one(const float* img, int w, int h, float x, float y, float scale, float orientation,
                         uint8_t* out, hipStream_t st);

}  // namespace siftmi
