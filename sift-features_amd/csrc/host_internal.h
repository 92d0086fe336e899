// Host-side types shared by pipeline.cpp (plan, pyramid, chunk pipeline) and
// api.cpp (the C ABI): error plumbing, owning device / pinned buffers, the
// pyramid plan, the per-chunk slot and the context.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sift_mi.h"
#include "geometry.h"
#include "result_state.h"
#include "sift_common.h"
#include "sift_kernels.h"

namespace siftmi {

inline thread_local std::string g_err;

inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return fail(SIFT_MI_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define CHK(expr)            \
    do {                     \
        int rc_ = (expr);    \
        if (rc_) return rc_; \
    } while (0)

// bumped by every device / pinned (re)allocation and release: a captured
// graph (single-chunk replay) is valid only while it is unchanged
inline std::atomic<uint64_t> g_alloc_gen{0};

// Owning device buffer (grow-only through ensure; freed with its owner).
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {  // o takes the old buffer and frees it with itself
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    ~DevBuf() { release(); }
    int ensure(size_t n) {
        if (n <= cap && p) return 0;
        g_alloc_gen++;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        if (hipMalloc(&p, bytes) != hipSuccess) {
            p = nullptr;
            return fail(SIFT_MI_ENOMEM, "hipMalloc(" + std::to_string(bytes) + ") failed");
        }
        cap = std::max<size_t>(n, 1);
        return 0;
    }
    void release() {
        if (p) {
            g_alloc_gen++;
            (void)hipFree(p);
        }
        p = nullptr;
        cap = 0;
    }
};

// d = n elements of host memory at src, enqueued on st; and n elements of d
// to host memory at dst, waited for.
template <class T>
int upload(DevBuf<T>& d, const T* src, size_t n, hipStream_t st) {
    CHK(d.ensure(n));
    HIPCHK(hipMemcpyAsync(d.p, src, n * sizeof(T), hipMemcpyHostToDevice, st));
    return 0;
}
template <class T>
int download(T* dst, const DevBuf<T>& d, size_t n, hipStream_t st) {
    HIPCHK(hipMemcpyAsync(dst, d.p, n * sizeof(T), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

// Grows d to at least n elements keeping its first `used` elements (device copy
// on stream st, synchronised).
template <class T>
int grow_keep(DevBuf<T>& d, size_t n, size_t used, hipStream_t st) {
    if (n <= d.cap && d.p) return 0;
    DevBuf<T> nd;
    CHK(nd.ensure(std::max(n, 2 * d.cap)));
    if (used && d.p) HIPCHK(hipMemcpyAsync(nd.p, d.p, used * sizeof(T), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    d = std::move(nd);
    return 0;
}

// Owning pinned host buffer.
template <class T>
struct PinBuf {
    T* p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    PinBuf(PinBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    PinBuf& operator=(PinBuf&& o) noexcept {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    ~PinBuf() { release(); }
    int ensure(size_t n, bool keep = false) {
        if (n <= cap && p) return 0;
        size_t ncap = std::max<size_t>({n, 1, cap * 2});
        g_alloc_gen++;
        T* q = nullptr;
        if (hipHostMalloc(&q, ncap * sizeof(T), hipHostMallocDefault) != hipSuccess)
            return fail(SIFT_MI_ENOMEM, "hipHostMalloc failed");
        if (keep && p && cap) std::memcpy(q, p, cap * sizeof(T));
        if (p) (void)hipHostFree(p);
        p = q;
        cap = ncap;
        return 0;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// Device tables of one resize (both axes), taps padded with zero weights.
struct IpTabDev {
    DevBuf<int> xl, yl;
    DevBuf<float> xw, yw;
    int xtaps = 0, ytaps = 0;
    int upload(int sw, int sh, int dw, int dh, float support, int min_taps, hipStream_t st);
    IpResizeTab tab() const { return IpResizeTab{xl.p, xw.p, yl.p, yw.p}; }
};

struct ResizeTabDev {
    DevBuf<int> xofs, yofs;
    DevBuf<float> xa0, xa1, ya0, ya1;
    ResizeTab tab{};
    int upload(int sw, int sh, int dw, int dh, hipStream_t st);
};

// Frame geometry + pyramid arena for `chunk` frames of w x h.
struct Plan : OctaveGeom {
    uint32_t w = 0, h = 0, chunk = 0;
    int max_oct = 0;  // the context's max_octaves the plan was built for
    DevBuf<float> arena[2];  // per lane: [G_0 | D_0 | G_1 | D_1 ...], each chunk-major
    int profile = SIFT_MI_PROFILE_OPENCV;
    ResizeTabDev seed_tab;  // OpenCV profile
    IpTabDev seed_iptab;    // Imageproc profile
    DevBuf<const float*> d_gauss[2];  // per lane
    DevBuf<size_t> d_gstride;
    DevBuf<int> d_ow, d_oh, d_opitch;
    BlurTaps seed_taps{};
    int seed_r = 0;
    BlurTaps oct_taps[kImagesPerOctave]{};
    int oct_r[kImagesPerOctave]{};
    uint64_t algo_bytes_per_frame = 0;

    float* gauss(int o, int lane = 0) { return arena[lane].p + goff[o]; }
    float* dog(int o, int lane = 0) { return arena[lane].p + doff[o]; }
    size_t gstride(int o) const { return (size_t)kImagesPerOctave * P[o]; }
    size_t dstride(int o) const { return (size_t)kDogPerOctave * P[o]; }
    OctaveView view(int lane) const { return {d_gauss[lane].p, d_gstride.p, d_ow.p, d_oh.p, d_opitch.p}; }
};

// Slot::counters, in uint32 words:
//   [4 stage counts | m frame starts | m per-frame outputs | kTailWords | kDescWorkWords]
// Every accessor is a word offset (into the device counters or their host
// copy).  The tail words are the counters of the tail octaves' own region
// (Slot::early) and the two-ended extremum append's back count
// (PathOpts::large_first).
struct CounterLayout {
    uint32_t m;  // frames of the chunk
    static constexpr uint32_t kStageWords = 4, kTailWords = 4;
    uint32_t cand() const { return 0; }
    uint32_t ext() const { return 1; }
    uint32_t kp() const { return 2; }
    uint32_t out() const { return 3; }
    uint32_t starts() const { return kStageWords; }
    uint32_t out_cnt() const { return kStageWords + m; }
    uint32_t tail() const { return kStageWords + 2 * m; }
    uint32_t tail_cand() const { return tail(); }
    uint32_t tail_ext() const { return tail() + 1; }
    uint32_t ext_back() const { return tail() + 3; }
    uint32_t work() const { return tail() + kTailWords; }  // descriptor work queues
    uint32_t host_words() const { return work(); }         // what finalize_chunk reads
    uint32_t device_words() const { return work() + kDescWorkWords; }
    // the zeroed words after the frame plan (k_chunk_init, k_seed_pair's reset)
    uint32_t reset_words() const { return kTailWords + kDescWorkWords; }
};

// Per-chunk state that outlives the enqueue: device counters, final outputs
// and the events of one in-flight chunk.  Two slots alternate, so chunk k+1's
// kernels run while the host waits for chunk k and copies its results out.
struct Slot {
    DevBuf<uint32_t> counters;  // CounterLayout{m}
    PinBuf<uint32_t> h_counts;
    DevBuf<OutKp> out_kp;
    DevBuf<uint8_t> out_desc;
    DevBuf<uint64_t> out_key;
    DevBuf<uint8_t> desc_kp;  // one-frame calls: descriptors in keypoint index order (Slot::desc_first)
    hipEvent_t ev[7] = {};   // stage boundaries on the compute stream (ev[6] = chunk done)
    hipEvent_t copied = {};  // results copied to the host (copy stream)
    hipEvent_t ordered = {};  // desc_first: the ordering stage done (lane 1's stream)
    bool pending_copy = false;
    bool detected = false;  // this chunk's detection is enqueued (stage overlap: inside the pyramid)
    uint32_t fused_mask = 0;  // octaves detected by k_blur_detect (with their blur 5) in the pyramid
    bool graph_run = false;   // the chunk was a graph replay: only ev[0] / ev[6] were recorded
    // ev[0..5] recorded: the one-lane mode times the stages (a marker packet
    // costs ~7 us of the stream's timeline; two-lane calls record only ev[6])
    bool staged = false;
    hipEvent_t oriented = {};  // desc_first: the keypoints are oriented (fork to lane 1's stream)
    // single-chunk calls with octave overlap: refinement + orientation of the
    // octaves below the tail run on the aux stream beside the tail (early),
    // the tail octaves' candidates / extrema in their own region (cand_b,
    // ext_b; counters at CounterLayout::tail_cand / tail_ext)
    bool early = false;
    // one-frame early calls without a limit: the descriptors are computed in
    // keypoint index order (desc_kp) while lane 1's stream orders the
    // keypoints; k_gather_out then writes the outputs in emission order
    bool desc_first = false;
    // early, two lanes: the aux stream's join event (oct_ev[lane][kTailMaxOct])
    // is recorded but the lane stream has not waited for it yet; the keypoint
    // stage either waits first or, with desc_first, runs the descriptors on
    // the aux stream itself (no cross-stream hop before them)
    bool join_pending = false;
    // the chunk's counter reset is launched right after the seed pass
    // (run_pyramid) instead of before it: the seed does not touch them
    bool init_pending = false;
    uint32_t bcb = 0;
    DevBuf<uint64_t> cand_b;
    DevBuf<ExtRec> ext_b;
    uint32_t m = 0, frame_base = 0;
    uint32_t bc = 0, be = 0, bk = 0;  // candidate / extremum / keypoint bounds used by this chunk
    // detection / description buffers of this slot's lane (the slot's chunks
    // run in its lane's stream order)
    DevBuf<uint64_t> cand;
    DevBuf<ExtRec> ext;
    DevBuf<KpRec> kp;
    DevBuf<uint64_t> keys_a, keys_b;
    DevBuf<uint32_t> vals_a, vals_b, fin;
    DevBuf<uint8_t> sort_tmp;
    DevBuf<uint32_t> seg_off, out_off;
    DevBuf<uint8_t> use_resp;

    CounterLayout layout() const { return CounterLayout{m}; }
};

// Pooled scratch of the segmented matcher (sift_mi_match_pairs_device and the
// host-array calls over it): grows on demand, freed with the context.
struct MatchScratch {
    DevBuf<uint8_t> desc;      // host-array calls: [query rows | train rows]
    DevBuf<uint32_t> table;    // MatchPair[n_pairs + 1] | norm blocks (uint2)
    PinBuf<uint32_t> h_table;
    DevBuf<int> nrm;           // per arena row: |row|^2 - 256 sum(row)
    DevBuf<unsigned long long> best, second;  // per (pair, query)
    DevBuf<unsigned long long> col;           // per (pair, train)
    DevBuf<int> tix, nb_idx;
    DevBuf<float> dist, nb_dist;
    PinBuf<int> h_tix, h_nb_idx;
    PinBuf<float> h_dist, h_nb_dist;
    // the guided matcher (sift_mi_match_pairs_guided_device, sift_mi_match_guided)
    DevBuf<OutKp> kps;         // sift_mi_match_guided: [query keypoints | train keypoints]
    DevBuf<float> models;      // per pair 9 f32
    PinBuf<float> h_models;
    DevBuf<float4> qterm, tterm;  // the gate's per (pair, query) / per (pair, train) terms
    DevBuf<uint32_t> culled;      // per tile: one byte per wave, 1 where it left at the cull
    DevBuf<unsigned long long> n_culled;
    PinBuf<unsigned long long> h_culled;
    uint64_t guided_tiles = 0, guided_culled = 0;  // sift_mi_guided_counters
    hipEvent_t t0 = nullptr, t1 = nullptr;  // around the kernels (sift_mi_stats.match_ms)
    ~MatchScratch() {
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
    }
};

// Pooled scratch of the geometric verification (sift_mi_verify_pairs_device,
// sift_mi_verify_matches): grows on demand, freed with the context.
struct VerifyScratch {
    DevBuf<OutKp> kps;  // sift_mi_verify_matches: [query keypoints | train keypoints]
    DevBuf<VerifyMatch> matches;
    DevBuf<VerifyPair> pairs;
    DevBuf<float4> rec;      // per match (x, y, X, Y)
    DevBuf<float> models;    // per (pair, hypothesis) 9 f32
    DevBuf<double> box;      // epipolar model: per pair the six f64 values of its box normalisation
    DevBuf<unsigned long long> best;  // per pair (count << 32 | ~hypothesis)
    DevBuf<VerifyModel> out;
    DevBuf<uint8_t> mask;
    // the progressive calls (sift_mi_verify_*_progressive*; prosac_growth.h)
    DevBuf<float> quality;     // per match, when the caller passes one
    DevBuf<uint32_t> growth;   // per match position its pair's T'
    DevBuf<uint32_t> perm;     // per rank position the caller's match
    DevBuf<uint2> rank_wgs;    // per workgroup of the ranking gather (pair, first match)
    PinBuf<uint32_t> h_growth;
    PinBuf<uint2> h_rank_wgs;
};

// Pooled scratch of the track builder (sift_mi_build_tracks_device): grows on
// demand, freed with the context.
struct TrackScratch {
    DevBuf<VerifyMatch> matches;
    DevBuf<uint8_t> keep;
    DevBuf<TrackPair> pairs;
    DevBuf<uint32_t> offs;  // per segment its first row
    DevBuf<uint32_t> parent, seg_of, label, row, sorted_label, sorted_row, start, end;
    DevBuf<uint8_t> confl, sort_tmp;
    DevBuf<uint2> bsum;
    DevBuf<uint32_t> totals, track_offsets;
    DevBuf<int32_t> track_of;
    DevBuf<TrackObs> obs;
    DevBuf<uint8_t> conflict;
    PinBuf<uint32_t> h_totals;
    hipEvent_t t0 = nullptr, t1 = nullptr;  // around the kernels
    double kernel_ms = 0;                   // sift_mi_track_counters
    uint64_t edges = 0;
    ~TrackScratch() {
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
    }
};

// Pooled scratch of the pair proposal (sift_mi_propose_pairs_device): grows on
// demand, freed with the context.
struct PairScratch {
    DevBuf<uint32_t> offs;   // per segment its first row, and the end of the last
    DevBuf<uint32_t> cnt;    // per segment min(rows, subset)
    DevBuf<uint8_t> sub_d;   // [n_segs * subset] gathered descriptor rows
    DevBuf<int> sub_m;       // their |row|^2 - 256 sum(row)
    DevBuf<uint32_t> score;  // [n_segs * n_segs]
    PinBuf<uint32_t> h_score;
    hipEvent_t t0 = nullptr, t1 = nullptr;  // around the kernels
    double kernel_ms = 0;                   // sift_mi_pair_counters
    uint64_t tiles = 0;
    ~PairScratch() {
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
    }
};

// Pooled scratch of the spread-limited selection (sift_mi_select_spread_device):
// grows on demand, freed with the context.  sel_kps / sel_desc are the compact
// arena sift_mi_selected_results hands out.
struct SelectScratch {
    DevBuf<uint32_t> tab;    // offs[n_segs + 1], sel_offs[n_segs + 1], then the radius workgroups' (segment, row)
    PinBuf<uint32_t> h_tab;  // its host image
    DevBuf<OutKp> in_kps;    // the one-frame host form's keypoints
    DevBuf<float> r2;        // per arena row
    DevBuf<uint32_t> rows, src;
    DevBuf<OutKp> sel_kps;
    DevBuf<uint8_t> sel_desc;
    size_t n_sel = 0;
    bool has_desc = false;
    hipEvent_t t0 = nullptr, t1 = nullptr;  // around the kernels
    double kernel_ms = 0;                   // sift_mi_select_counters
    uint64_t pair_tests = 0;
    ~SelectScratch() {
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
    }
};

}  // namespace siftmi

struct sift_mi_ctx {
    int device = 0;
    sift_mi_profile profile = SIFT_MI_PROFILE_OPENCV;
    hipStream_t own = nullptr;
    hipStream_t stream = nullptr;  // compute stream (own or the caller's)
    hipStream_t cstream = nullptr; // device->host result copies
    hipStream_t own2 = nullptr;    // compute stream of pipeline lane 1 (lane 0 runs on `stream`)
    hipStream_t aux[2] = {};       // per lane: blurs 4, 5 of each octave beside the next octave
    hipStream_t aux2 = nullptr;    // lane 0: blurs 4, 5 of octaves >= 1 while octave 0's fused pass runs
    hipEvent_t aux2_join = nullptr;
    hipStream_t dec = nullptr;     // JPEG batch decoding: a high-priority stream (its own hardware queue)
    hipEvent_t oct_ev[2][siftmi::kTailMaxOct + 1] = {};  // per lane: octave o's G_3 done / aux joined
    bool lanes_busy = false;       // this call keeps both pipeline lanes busy (no octave overlap then)
    siftmi::PathOpts opts;         // kernel-path switches (sift_mi_set_path_option)
    hipEvent_t fork = nullptr;     // orders lane 1 after / before the caller's stream
    int lanes = 2;                 // pipeline lanes (sift_mi_set_pipeline_lanes)
    uint32_t chunk_override = 0;
    uint32_t band_r = 0, band_n = 1;  // row band of the keypoint stages (sift_mi_set_row_band)
    siftmi::JpegBatchCache jpeg;      // sift_mi_decode_jpeg_batch buffers
    siftmi::DevBuf<uint32_t> band_flag;  // a refinement left the restricted rows (row bands)
    bool band_restricted = false;     // this call computes only the band's pyramid rows
    bool band_whole = false;          // re-run of a band on the whole-frame pyramid
    int exact_descriptors = 0;
    int max_octaves = 0;                    // sift_mi_set_max_octaves (0: the crate's formula)
    int count_samples = 0;                  // sift_mi_set_sample_counting (measurement only)
    siftmi::DevBuf<unsigned long long> samples;  // [0, 8): orientation, [8, 16): descriptor sample counters
    siftmi::Plan plan;
    siftmi::DevBuf<uint8_t> staging;  // host-sourced frames
    siftmi::Slot slot[2];  // slot = pipeline lane: chunk k runs on lane k & 1
    // per-frame high-water marks that size the next chunk's bounds
    double pf_cand = 0, pf_ext = 0, pf_kp = 0;
    double pf_cand_b = 0;  // the tail octaves' candidates / extrema (Slot::early)
    // device results of a whole batch (keep_on_device), concatenated in frame order
    siftmi::DevBuf<siftmi::OutKp> r_kp;
    siftmi::DevBuf<uint8_t> r_desc;
    siftmi::DevBuf<uint64_t> r_key;
    // host results (pinned)
    siftmi::PinBuf<siftmi::OutKp> h_kp;
    siftmi::PinBuf<uint8_t> h_desc;
    siftmi::PinBuf<uint64_t> h_key;
    // What the last producing call left and which calls may read it (result_state.h;
    // include/sift_mi.h "Call sequence").  The fields below it are details of a
    // state it admits, never consulted on their own.
    siftmi::ResultState rs;
    siftmi::ResultWhere call_dest = siftmi::ResultWhere::host;  // the call in progress: where its rows go
    size_t n_rows = 0;        // the call in progress: rows emitted so far (finalize_chunk)
    int res_slot = -1;        // rs.where == device: >= 0, that slot's outputs are the results (one chunk, no copy)
    int batch_arena = 0;      // rs.batch_readback: the arena the one chunk ran in
    // Single-chunk calls as a HIP graph (PathOpts::graph): the call's ~40
    // launches are captured the second time an identical call (same frames
    // pointer, geometry, bounds, modes, buffers) is seen, then replayed with
    // one hipGraphLaunch.
    struct GraphKey {
        siftmi::PathOpts opts;  // the switches decide what is captured
        const uint8_t* frames;
        size_t frame_pitch, stride;
        uint32_t m, w, h, bc, be, bk, bcb;
        int64_t limit;
        uint64_t gen;
        int keep, exact, samples, lanes, prof, maxo;
        hipStream_t st;
        bool operator==(const GraphKey& o) const { return std::memcmp(this, &o, sizeof o) == 0; }
    };
    GraphKey gkey{}, gseen{};
    bool gkey_ok = false, gseen_ok = false;
    bool g_early = false;      // the captured chunk's host-side flags
    uint32_t g_fused = 0;
    hipGraph_t graph = nullptr;
    hipGraphExec_t gexec = nullptr;
    uint32_t batch_frames = 0;  // rs.batch_readback: its frames
    siftmi::MatchScratch match;
    siftmi::VerifyScratch verify;
    siftmi::TrackScratch tracks;
    siftmi::PairScratch pairs;
    siftmi::SelectScratch select;
    sift_mi_stats stats{};
};

// pipeline.cpp, called by the C ABI (api.cpp); internal to the library
#pragma GCC visibility push(hidden)
namespace siftmi {

constexpr uint32_t kMaxChunk = 256;  // frames per chunk (one workgroup plans the output: k_limit_plan)

int sync_lanes(sift_mi_ctx* c);
int set_device(sift_mi_ctx* c);
int check_frame_args(uint32_t w, uint32_t h, size_t stride);
// Every reason to refuse an extraction for its arguments, before a buffer is touched
int check_extract_args(const sift_mi_ctx* c, uint32_t n, uint32_t w, uint32_t h, size_t stride, int64_t limit);
// features_limit under row bands (sift_mi_set_row_band)
int check_band_limit(const sift_mi_ctx* c, int64_t limit);
int upload_frames(sift_mi_ctx* c, const uint8_t* const* frames, uint32_t n, uint32_t w, uint32_t h, size_t stride);
int ensure_plan(sift_mi_ctx* c, uint32_t w, uint32_t h, uint32_t chunk);
// Stage 1: Gaussian scale space (+ DoG when `full`) of n device-resident u8 frames
int run_pyramid(sift_mi_ctx* c, int lane, const uint8_t* d_frames, size_t frame_pitch, size_t row_stride,
                uint32_t n, bool full, int detect_slot = -1, int cand_slot = -1);
// Single chunk, synchronous (sift_with_precomputed)
int run_chunk_sync(sift_mi_ctx* c, const uint8_t* d_frames, size_t frame_pitch, size_t stride, uint32_t m,
                   int64_t limit, bool pyramid, size_t* offsets);
// Device-resident batch pipeline; `call` says whose frames these are (host frames
// staged by the caller, or the caller's device frames: result_state.h)
int extract_device(sift_mi_ctx* c, ProducingCall call, const uint8_t* d_frames, size_t frame_pitch, uint32_t n,
                   uint32_t w, uint32_t h, size_t stride, int64_t limit, size_t* offsets);

}  // namespace siftmi
#pragma GCC visibility pop
