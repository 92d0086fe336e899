// libsift_mi.so: the C ABI of include/sift_mi.h over the pipeline
// (pipeline.cpp) and the HIP kernels in this directory, the contexts' stream
// pool and the stand-alone Processing ops.
#include <cmath>
#include <mutex>
#include <new>
#include <thread>

#include "host_internal.h"
#include "pair_propose.h"
#include "prosac_growth.h"
#include "select_rule.h"

using namespace siftmi;

namespace {
// Process-wide pool of the contexts' streams (per device, in creation
// order).  HIP maps streams onto a few hardware queues (GPU_MAX_HW_QUEUES,
// 4 by default) as they are created; a context created after another was
// destroyed would otherwise get a different, possibly colliding mapping
// (measured: one 1080p frame per call 0.69 ms in a fresh process, 0.89 ms
// after a closed batch context -- the octave overlap's two streams had landed
// on one queue).  A closed context returns its streams here; the next one
// takes the same stream objects back, so every context sees the queue
// mapping of the first.
struct StreamPool {
    std::mutex mu;
    std::vector<std::vector<hipStream_t>> free_sets[64];  // per device: sets of kCtxStreams
};
StreamPool& stream_pool() {
    static StreamPool* p = new StreamPool();  // never destroyed: streams live until process exit
    return *p;
}
// the order matters for the queue mapping: lane 0, lane 1, lane 0's aux,
// the copy stream, lane 1's aux, lane 0's second aux (with 4 queues the last
// two share the lanes' queues: lane 1's aux is used only when lane 1 is idle,
// the second aux only while lane 1's stream is: a one-lane / one-chunk call)
constexpr int kCtxStreams = 6;
bool take_streams(int dev, hipStream_t (&out)[kCtxStreams]) {
    StreamPool& P = stream_pool();
    {
        std::lock_guard<std::mutex> g(P.mu);
        auto& fs = P.free_sets[dev & 63];
        if (!fs.empty()) {
            for (int i = 0; i < kCtxStreams; i++) out[i] = fs.back()[i];
            fs.pop_back();
            return true;
        }
    }
    for (int i = 0; i < kCtxStreams; i++) {
        if (hipStreamCreateWithFlags(&out[i], hipStreamNonBlocking) != hipSuccess) {
            for (int k = 0; k < i; k++) (void)hipStreamDestroy(out[k]);
            return false;
        }
    }
    return true;
}
void give_streams(int dev, const hipStream_t (&in)[kCtxStreams]) {
    StreamPool& P = stream_pool();
    std::lock_guard<std::mutex> g(P.mu);
    P.free_sets[dev & 63].emplace_back(in, in + kCtxStreams);
}

// The events that only order the context's streams on the device (octave
// hand-overs, forks, joins, the one-frame path's oriented / ordered).
// (Measured: a device-scope release, hipEventReleaseToDevice, changed nothing
// -- 0.581-0.583 ms per 1080p frame either way; a signalling kernel still
// costs its stream ~5 us before the next one starts)
bool create_sync_events(sift_mi_ctx* c) {
    auto make = [&](hipEvent_t& e) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
        return hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    };
    bool ok = make(c->fork) && make(c->aux2_join);
    for (auto& lane : c->oct_ev)
        for (auto& e : lane) ok = ok && make(e);
    for (auto& S : c->slot) ok = ok && make(S.ordered) && make(S.oriented);
    return ok;
}

// Host copy of large results: split across threads (the copy is bound by
// page faults on freshly allocated destinations as much as by bandwidth).
void par_memcpy(void* dst, const void* src, size_t bytes) {
    constexpr size_t kPerThread = 4u << 20;
    const unsigned hw = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    const unsigned nt = (unsigned)std::min<size_t>(hw, bytes / kPerThread);
    if (nt <= 1) {
        std::memcpy(dst, src, bytes);
        return;
    }
    const size_t part = (bytes / nt + 4095) & ~(size_t)4095;
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; t++) {
        const size_t a = t * part;
        if (a >= bytes) break;
        const size_t b = std::min(bytes, a + part);
        th.emplace_back([=] { std::memcpy((char*)dst + a, (const char*)src + a, b - a); });
    }
    std::memcpy(dst, src, std::min(bytes, part));
    for (auto& x : th) x.join();
}

int octave_dims(const Plan& p, size_t o, uint32_t* w, uint32_t* h) {
    if (o >= (size_t)p.n_oct) return fail(SIFT_MI_EINVAL, "octave out of range");
    if (w) *w = (uint32_t)p.ow[o];
    if (h) *h = (uint32_t)p.oh[o];
    return 0;
}

// n consecutive pitched planes of octave o at src to the dense host array out
int read_planes(const Plan& p, int o, const float* src, int n, float* out) {
    HIPCHK(hipMemcpy2D(out, (size_t)p.ow[o] * sizeof(float), src, (size_t)p.opitch[o] * sizeof(float),
                       (size_t)p.ow[o] * sizeof(float), (size_t)n * p.oh[o], hipMemcpyDeviceToHost));
    return 0;
}

// image::imageops::resize on a host f32 image (Imageproc profile ops).
int ip_resize_op(sift_mi_ctx* c, const float* src, uint32_t w, uint32_t h, uint32_t dw, uint32_t dh, float support,
                 float* dst) {
    if (w == dw && h == dh) {  // image's resize copies when the size is unchanged
        std::memcpy(dst, src, sizeof(float) * (size_t)w * h);
        return 0;
    }
    IpTabDev tab;
    CHK(tab.upload((int)w, (int)h, (int)dw, (int)dh, support, 1, c->stream));
    DevBuf<float> a, t, b;
    CHK(upload(a, src, (size_t)w * h, c->stream));
    CHK(t.ensure((size_t)w * dh));
    CHK(b.ensure((size_t)dw * dh));
    launch_ip_resize_f32(a.p, (int)w, (int)h, tab.xl.p, tab.xw.p, tab.xtaps, tab.yl.p, tab.yw.p, tab.ytaps, t.p, b.p,
                         (int)dw, (int)dh, c->stream);
    return download(dst, b, (size_t)dw * dh, c->stream);
}

// No C++ exception leaves the JPEG entry points: the host side sizes vectors
// from the stream's headers.
template <class F>
int jpeg_guard(F&& body) {
    int rc = SIFT_MI_EINVAL;
    const char* what = "JPEG: exception";
    try {
        return body();
    } catch (const std::bad_alloc&) {
        rc = SIFT_MI_ENOMEM;
        what = "JPEG: host allocation failed";
    } catch (...) {
    }
    try {
        return fail(rc, what);
    } catch (...) {  // not even the message could be stored
        return rc;
    }
}
// No C++ exception leaves the match entry points (their host tables are
// sized by the caller's pair count).
template <class F>
int match_guard(F&& body) {
    int rc = SIFT_MI_EINVAL;
    const char* what = "match: exception";
    try {
        return body();
    } catch (const std::bad_alloc&) {
        rc = SIFT_MI_ENOMEM;
        what = "match: host allocation failed";
    } catch (...) {
    }
    try {
        return fail(rc, what);
    } catch (...) {
        return rc;
    }
}

// Grow-only pooled buffers of the matcher: half again on growth, so a
// sequence of slightly larger calls does not reallocate every time.
template <class B>
int pool(B& b, size_t n) {
    if (n <= b.cap && b.p) return 0;
    return b.ensure(std::max(n, b.cap + b.cap / 2));
}

int check_ratio(float ratio) {
    if (!(ratio >= 0.0f && ratio <= 1.0f)) return fail(SIFT_MI_EINVAL, "ratio must be 0 (no ratio test) or in (0, 1]");
    return 0;
}

// What a segmented match call covers: the arena rows of its segments, the
// (pair, query) slots, (pair, train) columns and 128 x 128 tiles of its pairs,
// and the words of its device table (the pairs, then the norm blocks).
struct MatchPlan {
    size_t row_base = 0, n_rows = 0, slots = 0, cols = 0, tiles = 0, n_blocks = 0, pair_words = 0, words = 0;
};

// Validates the segments and pairs of a segmented match call on device rows
// d_desc and fills P (P[p].qoff = pair p's first slot) and L.  With at least
// one slot it also fills the host table and grows the buffers every such call
// uses; nothing has run on the device yet.
int match_pairs_plan(sift_mi_ctx* c, const uint8_t* d_desc, const size_t* offsets, uint32_t n_segs,
                     const sift_mi_seg_pair* pairs, uint32_t n_pairs, std::vector<MatchPair>& P, MatchPlan& L) {
    constexpr size_t kMax = 0x7fffffff;
    if (((uintptr_t)d_desc & 15) != 0) return fail(SIFT_MI_EINVAL, "d_desc must be 16-byte aligned");
    for (uint32_t s = 0; s < n_segs; s++) {
        if (offsets[s + 1] < offsets[s]) return fail(SIFT_MI_EINVAL, "offsets decrease");
        if (offsets[s + 1] - offsets[s] > kMax) return fail(SIFT_MI_EINVAL, "segment longer than 2^31 - 1 rows");
    }
    L = MatchPlan{};
    L.row_base = offsets[0];
    L.n_rows = offsets[n_segs] - offsets[0];
    if (L.n_rows > kMax) return fail(SIFT_MI_EINVAL, "segments sum to more than 2^31 - 1 rows");
    P.assign((size_t)n_pairs + 1, MatchPair{});
    std::vector<char> used(n_segs, 0);
    size_t slots = 0, cols = 0, tiles = 0;
    for (uint32_t p = 0; p < n_pairs; p++) {
        const uint32_t qs = pairs[p].query_seg, ts = pairs[p].train_seg;
        if (qs >= n_segs || ts >= n_segs) return fail(SIFT_MI_EINVAL, "pair names a segment >= n_segs");
        MatchPair& m = P[p];
        m.qrow0 = (uint32_t)(offsets[qs] - L.row_base);
        m.nq = (uint32_t)(offsets[qs + 1] - offsets[qs]);
        m.trow0 = (uint32_t)(offsets[ts] - L.row_base);
        m.nt = (uint32_t)(offsets[ts + 1] - offsets[ts]);
        m.qoff = (uint32_t)slots;
        m.toff = (uint32_t)cols;
        m.tile0 = (uint32_t)tiles;
        slots += m.nq;
        cols += m.nt;
        if (m.nq && m.nt) {
            tiles += (size_t)((m.nq + 127) / 128) * ((m.nt + 127) / 128);
            used[qs] = used[ts] = 1;
        }
        if (slots > kMax || cols > kMax || tiles > kMax)
            return fail(SIFT_MI_EINVAL, "pairs sum to more than 2^31 - 1 queries, train rows or tiles");
    }
    P[n_pairs].qoff = (uint32_t)slots;
    P[n_pairs].toff = (uint32_t)cols;
    P[n_pairs].tile0 = (uint32_t)tiles;
    L.slots = slots;
    L.cols = cols;
    L.tiles = tiles;
    if (slots == 0) return 0;

    CHK(set_device(c));
    MatchScratch& M = c->match;
    // table: the pairs, then the 256-row blocks of the segments in use (their norms)
    L.pair_words = P.size() * (sizeof(MatchPair) / 4);
    for (uint32_t s = 0; s < n_segs; s++)
        if (used[s]) L.n_blocks += (offsets[s + 1] - offsets[s] + 255) / 256;
    L.words = L.pair_words + 2 * L.n_blocks;
    CHK(pool(M.h_table, L.words));
    std::memcpy(M.h_table.p, P.data(), L.pair_words * 4);
    uint32_t* blk = M.h_table.p + L.pair_words;
    for (uint32_t s = 0; s < n_segs; s++) {
        if (!used[s]) continue;
        for (size_t r = offsets[s]; r < offsets[s + 1]; r += 256) {
            *blk++ = (uint32_t)(r - L.row_base);
            *blk++ = (uint32_t)std::min<size_t>(256, offsets[s + 1] - r);
        }
    }
    CHK(pool(M.table, L.words));
    CHK(pool(M.nrm, L.n_rows));
    CHK(pool(M.best, slots));
    CHK(pool(M.second, slots));
    CHK(pool(M.col, cols));
    CHK(pool(M.tix, slots));
    CHK(pool(M.dist, slots));
    CHK(pool(M.h_tix, slots));
    CHK(pool(M.h_dist, slots));
    if (!M.t0) HIPCHK(hipEventCreate(&M.t0));
    if (!M.t1) HIPCHK(hipEventCreate(&M.t1));
    return 0;
}

// Runs a planned call on the context stream: uploads the table, `launch`es the
// kernels between the two events of sift_mi_stats.match_ms and leaves, per
// (pair, query) slot in pair order, the kept train index (-1: no match) and
// distance in c->match.h_tix / h_dist (with `neighbors`, both neighbours in
// h_nb_idx / h_nb_dist; with `guided`, the culled waves in h_culled),
// synchronised.
template <class Launch>
int match_pairs_execute(sift_mi_ctx* c, const MatchPlan& L, bool neighbors, bool guided, Launch&& launch) {
    MatchScratch& M = c->match;
    hipStream_t st = c->stream;
    const size_t slots = L.slots;
    HIPCHK(hipMemcpyAsync(M.table.p, M.h_table.p, L.words * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(M.t0, st));
    launch(st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(M.t1, st));
    HIPCHK(hipMemcpyAsync(M.h_tix.p, M.tix.p, slots * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(M.h_dist.p, M.dist.p, slots * sizeof(float), hipMemcpyDeviceToHost, st));
    if (neighbors) {
        HIPCHK(hipMemcpyAsync(M.h_nb_idx.p, M.nb_idx.p, 2 * slots * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(M.h_nb_dist.p, M.nb_dist.p, 2 * slots * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    if (guided)
        HIPCHK(hipMemcpyAsync(M.h_culled.p, M.n_culled.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, M.t0, M.t1) == hipSuccess) c->stats.match_ms += ms;
    return 0;
}

// The segmented matcher on device rows d_desc (match_pairs_plan, then
// launch_match_pairs through match_pairs_execute).
int match_pairs_run(sift_mi_ctx* c, const uint8_t* d_desc, const size_t* offsets, uint32_t n_segs,
                    const sift_mi_seg_pair* pairs, uint32_t n_pairs, float ratio, int cross_check, bool neighbors,
                    std::vector<MatchPair>& P) {
    MatchPlan L;
    CHK(match_pairs_plan(c, d_desc, offsets, n_segs, pairs, n_pairs, P, L));
    if (L.slots == 0) return 0;
    MatchScratch& M = c->match;
    if (neighbors) {
        CHK(pool(M.nb_idx, 2 * L.slots));
        CHK(pool(M.nb_dist, 2 * L.slots));
        CHK(pool(M.h_nb_idx, 2 * L.slots));
        CHK(pool(M.h_nb_dist, 2 * L.slots));
    }
    CHK(match_pairs_execute(c, L, neighbors, false, [&](hipStream_t st) {
        launch_match_pairs(d_desc + L.row_base * kDescSize, reinterpret_cast<const MatchPair*>(M.table.p), (int)n_pairs,
                           (uint32_t)L.tiles, (uint32_t)L.slots, (uint32_t)L.cols,
                           reinterpret_cast<const uint2*>(M.table.p + L.pair_words), (uint32_t)L.n_blocks,
                           cross_check ? 1 : 0, ratio, M.nrm.p, M.best.p, M.second.p, M.col.p, M.tix.p, M.dist.p,
                           neighbors ? M.nb_idx.p : nullptr, neighbors ? M.nb_dist.p : nullptr, st);
    }));
    c->stats.match_tiles += L.tiles;
    return 0;
}

int check_guided(int model_kind, const sift_mi_guided_params* p, const float* models, size_t n_pairs) {
    if (model_kind != SIFT_MI_MODEL_HOMOGRAPHY && model_kind != SIFT_MI_MODEL_FUNDAMENTAL)
        return fail(SIFT_MI_EINVAL, "unknown model kind");
    if (!(std::isfinite(p->threshold) && p->threshold > 0.0f))
        return fail(SIFT_MI_EINVAL, "threshold must be finite and > 0");
    CHK(check_ratio(p->ratio));
    if (!(p->max_distance >= 0.0f)) return fail(SIFT_MI_EINVAL, "max_distance must be 0 (no cap) or > 0");
    for (size_t i = 0; i < n_pairs * 9; i++)
        if (!std::isfinite(models[i])) return fail(SIFT_MI_EINVAL, "model entry not finite");
    return 0;
}

// The guided matcher on device rows d_desc and device keypoints d_kps of the
// same arena (with d_kps null, the host keypoints h_query / h_train of its two
// segments): every check on the host first, then match_pairs_run's sequence
// with launch_match_pairs_guided.  models: n_pairs * 9 host f32.
int match_guided_run(sift_mi_ctx* c, const uint8_t* d_desc, const OutKp* d_kps, const size_t* offsets, uint32_t n_segs,
                     const sift_mi_seg_pair* pairs, uint32_t n_pairs, int model_kind, const float* models,
                     const sift_mi_guided_params* prm, std::vector<MatchPair>& P, const OutKp* h_query = nullptr,
                     const OutKp* h_train = nullptr) {
    CHK(check_guided(model_kind, prm, models, n_pairs));
    if (((uintptr_t)d_kps & 3) != 0) return fail(SIFT_MI_EINVAL, "d_kps must be 4-byte aligned");
    MatchPlan L;
    CHK(match_pairs_plan(c, d_desc, offsets, n_segs, pairs, n_pairs, P, L));
    if (L.slots == 0) return 0;
    MatchScratch& M = c->match;
    const size_t n_models = (size_t)n_pairs * 9;
    CHK(pool(M.h_models, n_models));
    CHK(pool(M.models, n_models));
    CHK(pool(M.qterm, L.slots));
    CHK(pool(M.tterm, L.cols));
    CHK(pool(M.culled, L.tiles));
    CHK(pool(M.n_culled, 1));
    CHK(pool(M.h_culled, 1));
    hipStream_t st = c->stream;
    if (!d_kps) {  // host keypoints (two segments) as the context's own arena
        const size_t nq = offsets[1], nt = offsets[2] - offsets[1];
        CHK(pool(M.kps, nq + nt));
        if (nq) HIPCHK(hipMemcpyAsync(M.kps.p, h_query, nq * sizeof(OutKp), hipMemcpyHostToDevice, st));
        if (nt) HIPCHK(hipMemcpyAsync(M.kps.p + nq, h_train, nt * sizeof(OutKp), hipMemcpyHostToDevice, st));
        d_kps = M.kps.p;
    }
    std::memcpy(M.h_models.p, models, n_models * sizeof(float));
    HIPCHK(hipMemcpyAsync(M.models.p, M.h_models.p, n_models * sizeof(float), hipMemcpyHostToDevice, st));
    const int cull = c->opts.guided_cull;
    CHK(match_pairs_execute(c, L, false, true, [&](hipStream_t s) {
        launch_match_pairs_guided(d_desc + L.row_base * kDescSize, d_kps + L.row_base,
                                  reinterpret_cast<const MatchPair*>(M.table.p), (int)n_pairs, (uint32_t)L.tiles,
                                  (uint32_t)L.slots, (uint32_t)L.cols,
                                  reinterpret_cast<const uint2*>(M.table.p + L.pair_words), (uint32_t)L.n_blocks,
                                  model_kind == SIFT_MI_MODEL_FUNDAMENTAL, M.models.p, prm->threshold, cull,
                                  prm->cross_check ? 1 : 0, prm->ratio, prm->max_distance, M.nrm.p, M.best.p,
                                  M.second.p, M.col.p, M.qterm.p, M.tterm.p, M.culled.p, M.n_culled.p, M.tix.p,
                                  M.dist.p, s);
    }));
    M.guided_tiles += L.tiles;
    M.guided_culled += *M.h_culled.p;
    return 0;
}

// The kept slots of match_pairs_run as sift_mi_match rows, pair after pair.
int match_pairs_collect(const sift_mi_ctx* c, const std::vector<MatchPair>& P, sift_mi_match* out, size_t cap,
                        size_t* pair_offsets) {
    const size_t n_pairs = P.size() - 1, slots = P[n_pairs].qoff;
    const int* tix = c->match.h_tix.p;
    const float* dist = c->match.h_dist.p;
    size_t n = 0;
    for (size_t i = 0; i < slots; i++) n += tix[i] >= 0;
    if (cap < n || (n && !out)) {
        pair_offsets[n_pairs] = n;
        return fail(SIFT_MI_EINVAL, "cap < number of matches (pair_offsets[n_pairs])");
    }
    size_t k = 0;
    for (size_t p = 0; p < n_pairs; p++) {
        pair_offsets[p] = k;
        for (uint32_t i = 0; i < P[p].nq; i++) {
            const size_t s = (size_t)P[p].qoff + i;
            if (tix[s] >= 0) out[k++] = sift_mi_match{(int32_t)i, tix[s], dist[s]};
        }
    }
    pair_offsets[n_pairs] = k;
    return 0;
}

// Host descriptor arrays as the two segments of the context's own arena.
int match_upload(sift_mi_ctx* c, const uint8_t* query, size_t nq, const uint8_t* train, size_t nt) {
    CHK(set_device(c));
    MatchScratch& M = c->match;
    CHK(pool(M.desc, (nq + nt) * kDescSize));
    if (nq) HIPCHK(hipMemcpyAsync(M.desc.p, query, nq * kDescSize, hipMemcpyHostToDevice, c->stream));
    if (nt) HIPCHK(hipMemcpyAsync(M.desc.p + nq * kDescSize, train, nt * kDescSize, hipMemcpyHostToDevice, c->stream));
    return 0;
}

static_assert(sizeof(VerifyMatch) == sizeof(sift_mi_match) && sizeof(VerifyModel) == sizeof(sift_mi_homography) &&
                  sizeof(VerifyModel) == sizeof(sift_mi_fundamental) && sizeof(OutKp) == sizeof(sift_mi_keypoint),
              "verify.hip's and verify_epipolar.hip's records are the C ABI's");

enum class VerifyKind { Homography, Fundamental };

int check_ransac(const sift_mi_ransac_params* p) {
    if (!(std::isfinite(p->threshold) && p->threshold > 0.0f))
        return fail(SIFT_MI_EINVAL, "threshold must be finite and > 0");
    if (p->iterations < 1 || p->iterations > 65536) return fail(SIFT_MI_EINVAL, "iterations must be 1..65536");
    if (p->refit_rounds > 8) return fail(SIFT_MI_EINVAL, "refit_rounds must be 0..8");
    return 0;
}

// Verification of the pairs' matches on device keypoints d_kps: checks every
// segment, pair and match index on the host (no kernel sees an index outside
// its segment), uploads the matches (and, with d_kps null, the host keypoints
// h_query / h_train of the two segments), runs the launch sequence on the context
// stream and returns once models / inliers are written.  `models` receives
// n_pairs sift_mi_homography or sift_mi_fundamental records (one layout).
// sampling Progressive: the qualities (`quality`, or with it null the matches'
// distance) are checked on the host as well, the growth table of every pair and
// the ranking gather's workgroup list are built in pinned scratch and uploaded.
enum class VerifySampling { Uniform, Progressive };

int verify_run(sift_mi_ctx* c, VerifyKind kind, const OutKp* d_kps, const size_t* offsets, uint32_t n_segs,
               const sift_mi_seg_pair* pairs, uint32_t n_pairs, const sift_mi_match* matches,
               const size_t* pair_offsets, const sift_mi_ransac_params* prm, void* models,
               uint8_t* inliers, const OutKp* h_query = nullptr, const OutKp* h_train = nullptr,
               VerifySampling sampling = VerifySampling::Uniform, const float* quality = nullptr) {
    constexpr size_t kMax = 0x7fffffff;
    CHK(check_ransac(prm));
    if (((uintptr_t)d_kps & 3) != 0) return fail(SIFT_MI_EINVAL, "d_kps must be 4-byte aligned");
    for (uint32_t s = 0; s < n_segs; s++) {
        if (offsets[s + 1] < offsets[s]) return fail(SIFT_MI_EINVAL, "offsets decrease");
        if (offsets[s + 1] - offsets[s] > kMax) return fail(SIFT_MI_EINVAL, "segment longer than 2^31 - 1 rows");
    }
    const size_t row_base = offsets[0];
    if (offsets[n_segs] - row_base > kMax) return fail(SIFT_MI_EINVAL, "segments sum to more than 2^31 - 1 rows");
    for (uint32_t p = 0; p < n_pairs; p++)
        if (pair_offsets[p + 1] < pair_offsets[p]) return fail(SIFT_MI_EINVAL, "pair_offsets decrease");
    const size_t m_base = pair_offsets[0], total = pair_offsets[n_pairs] - m_base;
    if (total > kMax) return fail(SIFT_MI_EINVAL, "more than 2^31 - 1 matches");
    if (total && (!matches || !inliers)) return fail(SIFT_MI_EINVAL, "null argument");
    const uint32_t bpp = (prm->iterations + 255) / 256;
    // the epipolar models kernel runs 64 hypotheses per workgroup
    if ((size_t)n_pairs * bpp * (kind == VerifyKind::Fundamental ? 4 : 1) > kMax)
        return fail(SIFT_MI_EINVAL, "pairs x iterations too large");
    if (n_pairs == 0) return 0;
    std::vector<VerifyPair> P(n_pairs);
    for (uint32_t p = 0; p < n_pairs; p++) {
        const uint32_t qs = pairs[p].query_seg, ts = pairs[p].train_seg;
        if (qs >= n_segs || ts >= n_segs) return fail(SIFT_MI_EINVAL, "pair names a segment >= n_segs");
        const size_t nq = offsets[qs + 1] - offsets[qs], nt = offsets[ts + 1] - offsets[ts];
        for (size_t i = pair_offsets[p]; i < pair_offsets[p + 1]; i++) {
            const sift_mi_match& mt = matches[i];
            if (mt.query_idx < 0 || (size_t)mt.query_idx >= nq || mt.train_idx < 0 || (size_t)mt.train_idx >= nt)
                return fail(SIFT_MI_EINVAL, "match index outside its pair's segment (pair " + std::to_string(p) + ")");
        }
        P[p] = VerifyPair{(uint32_t)(pair_offsets[p] - m_base), (uint32_t)(pair_offsets[p + 1] - pair_offsets[p]),
                          (uint32_t)(offsets[qs] - row_base), (uint32_t)(offsets[ts] - row_base)};
    }
    const bool progressive = sampling == VerifySampling::Progressive;
    size_t n_wgs = 0;
    if (progressive) {
        const int bad = !total ? 0
                        : quality ? prosac::check_quality(quality + m_base, sizeof(float), total)
                                  : prosac::check_quality(&matches[m_base].distance, sizeof(sift_mi_match), total);
        if (bad)
            return fail(SIFT_MI_EINVAL, std::string(quality ? "quality" : "match distance") +
                                            (bad == 1 ? " must be finite" : " must have its sign bit clear"));
        for (uint32_t p = 0; p < n_pairs; p++) n_wgs += (P[p].m + kVerifyRankRows - 1) / kVerifyRankRows;
        if (n_wgs > kMax) return fail(SIFT_MI_EINVAL, "pairs x matches too large");
    }

    CHK(set_device(c));
    VerifyScratch& V = c->verify;
    VerifyProgressive prog{};
    if (progressive) {
        const uint32_t k = kind == VerifyKind::Fundamental ? 8 : 4;
        CHK(pool(V.growth, total));
        CHK(pool(V.perm, total));
        CHK(pool(V.rank_wgs, n_wgs));
        if (quality) CHK(pool(V.quality, total));
        CHK(V.h_growth.ensure(total));
        CHK(V.h_rank_wgs.ensure(n_wgs));
        prosac::fill_tables(
            n_pairs, [&P](size_t p, uint32_t& m, uint32_t& first) { m = P[p].m, first = P[p].rec0; }, k,
            prm->iterations, V.h_growth.p);
        size_t w = 0;
        for (uint32_t p = 0; p < n_pairs; p++)
            for (uint32_t r = 0; r < P[p].m; r += kVerifyRankRows) V.h_rank_wgs.p[w++] = make_uint2(p, r);
        prog = VerifyProgressive{quality ? V.quality.p : nullptr, V.growth.p, V.rank_wgs.p, (uint32_t)n_wgs, V.perm.p};
    }
    CHK(pool(V.pairs, n_pairs));
    CHK(pool(V.matches, total));
    CHK(pool(V.rec, total));
    CHK(pool(V.models, (size_t)n_pairs * prm->iterations * 9));
    CHK(pool(V.best, n_pairs));
    if (kind == VerifyKind::Fundamental) CHK(pool(V.box, (size_t)n_pairs * 6));
    CHK(pool(V.out, n_pairs));
    CHK(pool(V.mask, total));
    hipStream_t st = c->stream;
    if (!d_kps) {  // host keypoints (two segments) as the context's own arena
        const size_t nq = offsets[1], nt = offsets[2] - offsets[1];
        CHK(pool(V.kps, nq + nt));
        if (nq) HIPCHK(hipMemcpyAsync(V.kps.p, h_query, nq * sizeof(OutKp), hipMemcpyHostToDevice, st));
        if (nt) HIPCHK(hipMemcpyAsync(V.kps.p + nq, h_train, nt * sizeof(OutKp), hipMemcpyHostToDevice, st));
        d_kps = V.kps.p;
    }
    HIPCHK(hipMemcpyAsync(V.pairs.p, P.data(), (size_t)n_pairs * sizeof(VerifyPair), hipMemcpyHostToDevice, st));
    if (total)
        HIPCHK(hipMemcpyAsync(V.matches.p, matches + m_base, total * sizeof(VerifyMatch), hipMemcpyHostToDevice, st));
    if (progressive && total) {
        HIPCHK(hipMemcpyAsync(V.growth.p, V.h_growth.p, total * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(V.rank_wgs.p, V.h_rank_wgs.p, n_wgs * sizeof(uint2), hipMemcpyHostToDevice, st));
        if (quality)
            HIPCHK(hipMemcpyAsync(V.quality.p, quality + m_base, total * sizeof(float), hipMemcpyHostToDevice, st));
    }
    const VerifyProgressive* pg = progressive ? &prog : nullptr;
    if (kind == VerifyKind::Fundamental)
        launch_verify_epipolar(d_kps + row_base, V.matches.p, V.pairs.p, (int)n_pairs, (uint32_t)total, prm->threshold,
                               prm->iterations, prm->seed, prm->refit_rounds, V.rec.p, V.box.p, V.models.p, V.best.p,
                               V.out.p, V.mask.p, st, pg);
    else
        launch_verify(d_kps + row_base, V.matches.p, V.pairs.p, (int)n_pairs, (uint32_t)total, prm->threshold,
                      prm->iterations, prm->seed, prm->refit_rounds, V.rec.p, V.models.p, V.best.p, V.out.p, V.mask.p,
                      st, pg);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(models, V.out.p, (size_t)n_pairs * sizeof(VerifyModel), hipMemcpyDeviceToHost, st));
    if (total) HIPCHK(hipMemcpyAsync(inliers + m_base, V.mask.p, total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

static_assert(sizeof(TrackObs) == sizeof(sift_mi_track_obs), "tracks.hip's record is the C ABI's");

// Tracks over the pairs' kept matches on device keypoints d_kps: checks every
// segment, pair and match index on the host (no kernel sees an index outside
// its segment), uploads the matches and the mask, runs launch_tracks on the
// context stream, reads the two counts back and then exactly the tracks'
// share of the result arrays.  d_kps is only read.
int tracks_run(sift_mi_ctx* c, const OutKp* d_kps, const size_t* offsets, uint32_t n_segs,
               const sift_mi_seg_pair* pairs, uint32_t n_pairs, const sift_mi_match* matches,
               const size_t* pair_offsets, const uint8_t* keep, const sift_mi_track_params* prm, int32_t* track_of,
               uint32_t* n_tracks, uint32_t* track_offsets, sift_mi_track_obs* obs, uint8_t* conflict) {
    constexpr size_t kMax = 0x7fffffff;
    if (prm->min_length < 2) return fail(SIFT_MI_EINVAL, "min_length must be >= 2");
    if (((uintptr_t)d_kps & 3) != 0) return fail(SIFT_MI_EINVAL, "d_kps must be 4-byte aligned");
    for (uint32_t s = 0; s < n_segs; s++)
        if (offsets[s + 1] < offsets[s]) return fail(SIFT_MI_EINVAL, "offsets decrease");
    const size_t row_base = offsets[0], n_rows = offsets[n_segs] - row_base;
    if (n_rows > kMax) return fail(SIFT_MI_EINVAL, "segments sum to more than 2^31 - 1 rows");
    for (uint32_t p = 0; p < n_pairs; p++)
        if (pair_offsets[p + 1] < pair_offsets[p]) return fail(SIFT_MI_EINVAL, "pair_offsets decrease");
    const size_t m_base = pair_offsets[0], total = pair_offsets[n_pairs] - m_base;
    if (total > kMax) return fail(SIFT_MI_EINVAL, "more than 2^31 - 1 matches");
    std::vector<TrackPair> P(n_pairs);
    for (uint32_t p = 0; p < n_pairs; p++) {
        const uint32_t qs = pairs[p].query_seg, ts = pairs[p].train_seg;
        if (qs >= n_segs || ts >= n_segs) return fail(SIFT_MI_EINVAL, "pair names a segment >= n_segs");
        const size_t nq = offsets[qs + 1] - offsets[qs], nt = offsets[ts + 1] - offsets[ts];
        for (size_t i = pair_offsets[p]; i < pair_offsets[p + 1]; i++) {
            const sift_mi_match& mt = matches[i];
            if (mt.query_idx < 0 || (size_t)mt.query_idx >= nq || mt.train_idx < 0 || (size_t)mt.train_idx >= nt)
                return fail(SIFT_MI_EINVAL, "match index outside its pair's segment (pair " + std::to_string(p) + ")");
        }
        P[p] = TrackPair{(uint32_t)(pair_offsets[p] - m_base), (uint32_t)(offsets[qs] - row_base),
                         (uint32_t)(offsets[ts] - row_base)};
    }
    uint64_t edges = total;
    if (keep) {
        edges = 0;
        for (size_t i = 0; i < total; i++) edges += keep[m_base + i] != 0;
    }
    *n_tracks = 0;
    track_offsets[0] = 0;
    if (n_rows == 0) return 0;

    CHK(set_device(c));
    TrackScratch& T = c->tracks;
    hipStream_t st = c->stream;
    const size_t cap = n_rows / 2 + 2, n_blocks = (n_rows + 255) / 256;
    std::vector<uint32_t> seg_rows(n_segs);
    for (uint32_t s = 0; s < n_segs; s++) seg_rows[s] = (uint32_t)(offsets[s] - row_base);
    const size_t tmp = track_sort_temp_bytes((uint32_t)n_rows);
    if (!tmp) return fail(SIFT_MI_EHIP, "radix sort temporary storage query failed");
    CHK(pool(T.matches, total));
    if (keep) CHK(pool(T.keep, total));
    CHK(pool(T.pairs, n_pairs));
    CHK(pool(T.offs, n_segs));
    for (DevBuf<uint32_t>* b : {&T.parent, &T.seg_of, &T.label, &T.row, &T.sorted_label, &T.sorted_row, &T.start, &T.end})
        CHK(pool(*b, n_rows));
    CHK(pool(T.confl, n_rows));
    CHK(pool(T.sort_tmp, tmp));
    CHK(pool(T.bsum, n_blocks));
    CHK(pool(T.totals, 2));
    CHK(pool(T.track_offsets, cap));
    CHK(pool(T.track_of, n_rows));
    CHK(pool(T.obs, n_rows));
    CHK(pool(T.conflict, cap));
    CHK(pool(T.h_totals, 2));
    if (!T.t0) HIPCHK(hipEventCreate(&T.t0));
    if (!T.t1) HIPCHK(hipEventCreate(&T.t1));

    HIPCHK(hipMemcpyAsync(T.offs.p, seg_rows.data(), (size_t)n_segs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (total) {  // (with no match the link kernel is not launched and nothing reads these)
        HIPCHK(hipMemcpyAsync(T.pairs.p, P.data(), (size_t)n_pairs * sizeof(TrackPair), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(T.matches.p, matches + m_base, total * sizeof(VerifyMatch), hipMemcpyHostToDevice, st));
        if (keep) HIPCHK(hipMemcpyAsync(T.keep.p, keep + m_base, total, hipMemcpyHostToDevice, st));
    }
    TrackLaunch L{};
    L.kps = d_kps + row_base;
    L.offs = T.offs.p;
    L.n_segs = n_segs;
    L.n_rows = (uint32_t)n_rows;
    L.matches = T.matches.p;
    L.keep = keep && total ? T.keep.p : nullptr;
    L.pairs = T.pairs.p;
    L.n_pairs = n_pairs;
    L.n_matches = (uint32_t)total;
    L.min_length = prm->min_length;
    L.drop_conflicts = prm->drop_conflicts ? 1 : 0;
    L.parent = T.parent.p;
    L.seg_of = T.seg_of.p;
    L.label = T.label.p;
    L.row = T.row.p;
    L.sorted_label = T.sorted_label.p;
    L.sorted_row = T.sorted_row.p;
    L.start = T.start.p;
    L.end = T.end.p;
    L.confl = T.confl.p;
    L.bsum = T.bsum.p;
    L.sort_temp = T.sort_tmp.p;
    L.sort_temp_bytes = tmp;
    L.totals = T.totals.p;
    L.track_of = T.track_of.p;
    L.track_offsets = T.track_offsets.p;
    L.obs = reinterpret_cast<TrackObs*>(T.obs.p);
    L.conflict = T.conflict.p;
    HIPCHK(hipEventRecord(T.t0, st));
    if (launch_tracks(L, st) != 0) return fail(SIFT_MI_EHIP, "the tracks' radix sort could not be enqueued");
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(T.t1, st));
    // the two counts first: they size the downloads of the other arrays
    HIPCHK(hipMemcpyAsync(T.h_totals.p, T.totals.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(track_of, T.track_of.p, n_rows * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint32_t nt = T.h_totals.p[0], nm = T.h_totals.p[1];
    if ((size_t)nt + 1 > cap || nm > n_rows) return fail(SIFT_MI_EHIP, "track counts out of range");
    HIPCHK(hipMemcpyAsync(track_offsets, T.track_offsets.p, ((size_t)nt + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost,
                          st));
    if (nt) HIPCHK(hipMemcpyAsync(conflict, T.conflict.p, nt, hipMemcpyDeviceToHost, st));
    if (nm) HIPCHK(hipMemcpyAsync(obs, T.obs.p, (size_t)nm * sizeof(TrackObs), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *n_tracks = nt;
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, T.t0, T.t1) == hipSuccess) T.kernel_ms += ms;
    T.edges += edges;
    return 0;
}

constexpr uint32_t kPairMaxSegs = 4096;  // a 64 MB score matrix

// Pair proposal on device rows d_desc and device keypoints d_kps of one
// arena: every check on the host first, then launch_pairs on the context
// stream between the two events of sift_mi_pair_counters; only the n_segs^2
// scores come back, and the proposal runs on them here (pair_propose.h).
int pairs_run(sift_mi_ctx* c, const uint8_t* d_desc, const OutKp* d_kps, const size_t* offsets, uint32_t n_segs,
              const sift_mi_pair_params* prm, uint32_t* scores, sift_mi_seg_pair* pairs, size_t cap, size_t* n_pairs) {
    constexpr size_t kMax = 0x7fffffff;
    if (prm->subset < 1 || prm->subset > kPairSubsetMax) return fail(SIFT_MI_EINVAL, "subset must be 1..128");
    CHK(check_ratio(prm->ratio));
    if (prm->min_matches < 1) return fail(SIFT_MI_EINVAL, "min_matches must be >= 1");
    if (n_segs > kPairMaxSegs) return fail(SIFT_MI_EINVAL, "more than 4096 segments");
    if (((uintptr_t)d_desc & 15) != 0) return fail(SIFT_MI_EINVAL, "d_desc must be 16-byte aligned");
    if (((uintptr_t)d_kps & 3) != 0) return fail(SIFT_MI_EINVAL, "d_kps must be 4-byte aligned");
    for (uint32_t s = 0; s < n_segs; s++)
        if (offsets[s + 1] < offsets[s]) return fail(SIFT_MI_EINVAL, "offsets decrease");
    const size_t row_base = offsets[0];
    if (offsets[n_segs] - row_base > kMax) return fail(SIFT_MI_EINVAL, "segments sum to more than 2^31 - 1 rows");
    if (n_segs <= 1) {
        if (n_segs && scores) scores[0] = 0;
        return 0;
    }
    const uint32_t h = prm->subset;
    const size_t n2 = (size_t)n_segs * n_segs, n_sub = (size_t)n_segs * h;
    std::vector<uint32_t> seg_rows((size_t)n_segs + 1);
    for (uint32_t s = 0; s <= n_segs; s++) seg_rows[s] = (uint32_t)(offsets[s] - row_base);

    CHK(set_device(c));
    PairScratch& S = c->pairs;
    hipStream_t st = c->stream;
    CHK(pool(S.offs, (size_t)n_segs + 1));
    CHK(pool(S.cnt, n_segs));
    CHK(pool(S.sub_d, n_sub * kDescSize));
    CHK(pool(S.sub_m, n_sub));
    CHK(pool(S.score, n2));
    CHK(pool(S.h_score, n2));
    if (!S.t0) HIPCHK(hipEventCreate(&S.t0));
    if (!S.t1) HIPCHK(hipEventCreate(&S.t1));
    HIPCHK(hipMemcpyAsync(S.offs.p, seg_rows.data(), seg_rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(S.t0, st));
    launch_pairs(d_kps + row_base, d_desc + row_base * kDescSize, S.offs.p, n_segs, h, prm->ratio, S.cnt.p, S.sub_d.p,
                 S.sub_m.p, S.score.p, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.t1, st));
    HIPCHK(hipMemcpyAsync(S.h_score.p, S.score.p, n2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, S.t0, S.t1) == hipSuccess) S.kernel_ms += ms;
    S.tiles += (uint64_t)n_segs * (n_segs - 1) / 2;
    if (scores) std::memcpy(scores, S.h_score.p, n2 * sizeof(uint32_t));
    const std::vector<sift_mi_seg_pair> out =
        propose_from_scores(S.h_score.p, n_segs, prm->min_matches, prm->max_partners);
    *n_pairs = out.size();
    if (cap < out.size()) return fail(SIFT_MI_EINVAL, "cap < number of proposed pairs (*n_pairs)");
    if (!out.empty()) std::memcpy(pairs, out.data(), out.size() * sizeof(sift_mi_seg_pair));
    return 0;
}

// Spread-limited selection on device keypoints d_kps (host keypoints h_kps
// instead when d_kps is null: the one-frame form) and optional device rows
// d_desc of one arena: every check and sel_offsets on the host first
// (select_rule.h), then launch_select on the context stream between the two
// events of sift_mi_select_counters; rows and, if asked for, radius2 come back.
int select_run(sift_mi_ctx* c, const OutKp* d_kps, const OutKp* h_kps, const uint8_t* d_desc, const size_t* offsets,
               uint32_t n_segs, const sift_mi_select_params* prm, size_t* sel_offsets, uint32_t* rows, size_t cap,
               float* radius2) {
    if (const char* msg = select_params_error(prm->limit, prm->c)) return fail(SIFT_MI_EINVAL, msg);
    if (const char* msg = select_arena_error(d_kps, d_desc, offsets, n_segs)) return fail(SIFT_MI_EINVAL, msg);
    select_fill_offsets(offsets, n_segs, prm->limit, sel_offsets);
    const size_t total = sel_offsets[n_segs];
    if (cap < total) return fail(SIFT_MI_EINVAL, "cap < number of kept rows (sel_offsets[n_segs])");
    const size_t row_base = offsets[0], n_rows = offsets[n_segs] - row_base;
    size_t n_wgs = 0;
    for (uint32_t s = 0; s < n_segs; s++)
        n_wgs += (offsets[s + 1] - offsets[s] + kSelectRowsPerWg - 1) / kSelectRowsPerWg;

    CHK(set_device(c));
    SelectScratch& S = c->select;
    hipStream_t st = c->stream;
    S.n_sel = 0;
    S.has_desc = d_desc != nullptr;
    if (total == 0) return 0;  // (then no segment has a row)
    const size_t n_off = (size_t)n_segs + 1, words = 2 * n_off + 2 * n_wgs;
    CHK(pool(S.h_tab, words));
    CHK(pool(S.tab, words));
    CHK(pool(S.r2, n_rows));
    CHK(pool(S.rows, total));
    CHK(pool(S.src, total));
    CHK(pool(S.sel_kps, total));
    if (d_desc) CHK(pool(S.sel_desc, total * kDescSize));
    if (h_kps) CHK(pool(S.in_kps, n_rows));
    if (!S.t0) HIPCHK(hipEventCreate(&S.t0));
    if (!S.t1) HIPCHK(hipEventCreate(&S.t1));
    uint32_t* h = S.h_tab.p;
    uint64_t tests = 0;
    size_t w = 2 * n_off;
    for (uint32_t s = 0; s <= n_segs; s++) {
        h[s] = (uint32_t)(offsets[s] - row_base);
        h[n_off + s] = (uint32_t)sel_offsets[s];
    }
    for (uint32_t s = 0; s < n_segs; s++) {
        const size_t n = offsets[s + 1] - offsets[s];
        tests += (uint64_t)n * n;
        for (size_t r = 0; r < n; r += kSelectRowsPerWg) {
            h[w++] = s;
            h[w++] = (uint32_t)r;
        }
    }
    HIPCHK(hipMemcpyAsync(S.tab.p, h, words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (h_kps) HIPCHK(hipMemcpyAsync(S.in_kps.p, h_kps, n_rows * sizeof(OutKp), hipMemcpyHostToDevice, st));
    SelectLaunch L{};
    L.kps = h_kps ? S.in_kps.p : d_kps + row_base;
    L.d = d_desc ? d_desc + row_base * kDescSize : nullptr;
    L.offs = S.tab.p;
    L.sel_offs = S.tab.p + n_off;
    L.wgs = reinterpret_cast<const uint2*>(S.tab.p + 2 * n_off);  // (an even word: 8-byte aligned)
    L.n_segs = n_segs;
    L.n_wgs = (uint32_t)n_wgs;
    L.n_rows = (uint32_t)n_rows;
    L.total = (uint32_t)total;
    L.limit = prm->limit;
    L.c = prm->c;
    L.r2 = S.r2.p;
    L.rows = S.rows.p;
    L.src = S.src.p;
    L.sel_kps = S.sel_kps.p;
    L.sel_d = d_desc ? S.sel_desc.p : nullptr;
    HIPCHK(hipEventRecord(S.t0, st));
    launch_select(L, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.t1, st));
    HIPCHK(hipMemcpyAsync(rows, S.rows.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (radius2) HIPCHK(hipMemcpyAsync(radius2, S.r2.p, n_rows * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, S.t0, S.t1) == hipSuccess) S.kernel_ms += ms;
    S.pair_tests += tests;
    S.n_sel = total;
    return 0;
}
}  // namespace

extern "C" {

const char* sift_mi_version(void) { return "sift_mi 0.5.0 (gfx950)"; }
const char* sift_mi_last_error(void) { return g_err.c_str(); }

int sift_mi_create(int device_ordinal, sift_mi_profile profile, sift_mi_ctx** out) {
    if (!out) return fail(SIFT_MI_EINVAL, "out is null");
    *out = nullptr;
    if (profile != SIFT_MI_PROFILE_OPENCV && profile != SIFT_MI_PROFILE_IMAGEPROC)
        return fail(SIFT_MI_EINVAL, "unknown profile");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SIFT_MI_ENODEV, "no HIP device");
    if (device_ordinal < 0 || device_ordinal >= ndev) return fail(SIFT_MI_ENODEV, "device ordinal out of range");
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device_ordinal));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SIFT_MI_ENODEV, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950");
    HIPCHK(hipSetDevice(device_ordinal));
    sift_mi_ctx* c = new sift_mi_ctx();
    c->device = device_ordinal;
    c->profile = profile;
    hipStream_t ss[kCtxStreams];
    if (!take_streams(device_ordinal, ss)) {
        delete c;
        return fail(SIFT_MI_EHIP, "hipStreamCreate failed");
    }
    c->own = ss[0];
    c->own2 = ss[1];
    c->aux[0] = ss[2];
    c->cstream = ss[3];
    c->aux[1] = ss[4];
    c->aux2 = ss[5];
    c->stream = c->own;
    bool ok = create_sync_events(c);
    for (auto& S : c->slot) {
        for (auto& e : S.ev) ok = ok && hipEventCreate(&e) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&S.copied, hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) {
        sift_mi_destroy(c);
        return fail(SIFT_MI_EHIP, "stream / event creation failed");
    }
    *out = c;
    return 0;
}

void sift_mi_destroy(sift_mi_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    // every stream that may still run work on this context's buffers first:
    // the caller's stream (sift_mi_set_stream), the context's own lane-0
    // stream (it goes back to the pool below), lane 1, both aux streams
    // (octave blurs 4, 5 and detection write the arenas) and the copy stream
    {
        const hipStream_t ss[] = {c->stream, c->own, c->own2, c->aux[0], c->aux[1], c->aux2, c->cstream, c->dec};
        for (hipStream_t s : ss)
            if (s) (void)hipStreamSynchronize(s);
    }
    auto destroy = [](hipEvent_t e) {
        if (e) (void)hipEventDestroy(e);
    };
    for (auto& S : c->slot) {
        for (auto& e : S.ev) destroy(e);
        destroy(S.copied);
        destroy(S.ordered);
        destroy(S.oriented);
    }
    destroy(c->fork);
    destroy(c->aux2_join);
    for (auto& lane : c->oct_ev)
        for (auto& e : lane) destroy(e);
    c->jpeg.release();  // (its events too)
    if (c->dec) (void)hipStreamDestroy(c->dec);
    if (c->gexec) (void)hipGraphExecDestroy(c->gexec);
    if (c->graph) (void)hipGraphDestroy(c->graph);
    if (c->own) {  // the streams go back to the pool (synchronised above)
        const hipStream_t ss[kCtxStreams] = {c->own, c->own2, c->aux[0], c->cstream, c->aux[1], c->aux2};
        give_streams(c->device, ss);
    }
    delete c;  // frees every buffer the context, its plan and its slots own
}

int sift_mi_set_stream(sift_mi_ctx* c, void* s) {
    if (!c) return fail(SIFT_MI_EINVAL, "ctx is null");
    c->stream = s ? (hipStream_t)s : c->own;
    return 0;
}

int sift_mi_set_chunk(sift_mi_ctx* c, uint32_t k) {
    if (!c) return fail(SIFT_MI_EINVAL, "ctx is null");
    c->chunk_override = k;
    return 0;
}

int sift_mi_set_max_octaves(sift_mi_ctx* c, int max_octaves) {
    if (!c || max_octaves < 0) return fail(SIFT_MI_EINVAL, "max_octaves must be >= 0");
    CHK(set_device(c));
    CHK(sync_lanes(c));
    c->max_octaves = max_octaves;  // the plan is rebuilt on the next call
    c->rs.set_max_octaves();
    return 0;
}

int sift_mi_set_exact_descriptors(sift_mi_ctx* c, int exact) {
    if (!c) return fail(SIFT_MI_EINVAL, "ctx is null");
    c->exact_descriptors = exact ? 1 : 0;
    return 0;
}

int sift_mi_set_pipeline_lanes(sift_mi_ctx* c, int lanes) {
    if (!c || (lanes != 1 && lanes != 2)) return fail(SIFT_MI_EINVAL, "lanes must be 1 or 2");
    CHK(set_device(c));
    CHK(sync_lanes(c));
    c->lanes = lanes;
    return 0;
}

int sift_mi_set_row_band(sift_mi_ctx* c, uint32_t band, uint32_t n_bands) {
    if (!c || n_bands == 0 || band >= n_bands) return fail(SIFT_MI_EINVAL, "band must be < n_bands, n_bands >= 1");
    c->band_r = band;
    c->band_n = n_bands;
    return 0;
}

int sift_mi_set_path_option(sift_mi_ctx* c, int option, int value) {
    if (!c) return fail(SIFT_MI_EINVAL, "ctx is null");
    CHK(set_device(c));
    CHK(sync_lanes(c));  // no chunk in flight sees a half-changed path
    PathOpts& o = c->opts;
    const bool b = value == 0 || value == 1;
    switch (option) {
        case SIFT_MI_PATH_TILE_BLUR: if (!b) break; o.tile_blur = value; return 0;
        case SIFT_MI_PATH_PAIR_BLUR: if (!b) break; o.pair = value; return 0;
        case SIFT_MI_PATH_SEED_PAIR: if (!b) break; o.seed_pair = value; return 0;
        case SIFT_MI_PATH_TAIL: if (!b) break; o.tail = value; return 0;
        case SIFT_MI_PATH_FUSED_DETECT: if (value < 0 || value > 2) break; o.fused_detect = value; return 0;
        case SIFT_MI_PATH_EARLY: if (!b) break; o.early = value; return 0;
        case SIFT_MI_PATH_DESC_FIRST: if (!b) break; o.desc_first = value; return 0;
        case SIFT_MI_PATH_GRAPH: if (!b) break; o.graph = value; return 0;
        case SIFT_MI_PATH_BAND_DRIFT: if (value < -kBandPatch || value > kBandDrift) break; o.band_drift = value; return 0;
        case SIFT_MI_PATH_BOUND_SHRINK: if (value < 1) break; o.bound_shrink = value; return 0;
        case SIFT_MI_PATH_LARGE_FIRST: if (!b) break; o.large_first = value; return 0;
        case SIFT_MI_PATH_ONESWEEP: if (value < 0 || value > 2) break; o.onesweep = value; return 0;
        case SIFT_MI_PATH_BD_PAIR: if (value < 0 || value > 2) break; o.bd_pair = value; return 0;
        case SIFT_MI_PATH_BD_WAVES: if (value < 1024 || value > 65536) break; o.bd_waves = value; return 0;
        case SIFT_MI_PATH_CHUNK_MODE: if (value < 0 || value > 1) break; o.chunk_mode = value; return 0;
        case SIFT_MI_PATH_GUIDED_CULL: if (!b) break; o.guided_cull = value; return 0;
        default: return fail(SIFT_MI_EINVAL, "unknown path option");
    }
    return fail(SIFT_MI_EINVAL, "path option value out of range");
}

int sift_mi_set_keep_on_device(sift_mi_ctx* c, int keep) {
    if (!c) return fail(SIFT_MI_EINVAL, "ctx is null");
    c->rs.set_keep(keep != 0);  // the destination of later device-frame calls; the last result stays where it is
    return 0;
}

int sift_mi_extract_batch_device(sift_mi_ctx* c, const uint8_t* d_frames, size_t frame_pitch, uint32_t n,
                                 uint32_t w, uint32_t h, size_t stride, int64_t limit, size_t* offsets) {
    if (!c || !d_frames || n == 0) return fail(SIFT_MI_EINVAL, "bad arguments");
    if (frame_pitch < stride * (h - 1) + w && n > 1) return fail(SIFT_MI_EINVAL, "frame_pitch too small");
    CHK(check_extract_args(c, n, w, h, stride, limit));
    CHK(set_device(c));
    return extract_device(c, ProducingCall::extract_device, d_frames, frame_pitch, n, w, h, stride, limit, offsets);
}

int sift_mi_extract_batch(sift_mi_ctx* c, const uint8_t* const* frames, uint32_t n, uint32_t w, uint32_t h,
                          size_t stride, int64_t limit, size_t* offsets) {
    if (!c || !frames || n == 0) return fail(SIFT_MI_EINVAL, "bad arguments");
    CHK(check_extract_args(c, n, w, h, stride, limit));  // before the staging buffer is written
    CHK(set_device(c));
    CHK(upload_frames(c, frames, n, w, h, stride));
    // host frames: the rows go to the host whatever the keep setting says
    return extract_device(c, ProducingCall::extract, c->staging.p, (size_t)w * h, n, w, h, w, limit, offsets);
}

int sift_mi_extract(sift_mi_ctx* c, const uint8_t* pixels, uint32_t w, uint32_t h, size_t stride, int64_t limit,
                    size_t* n_keypoints) {
    if (!c || !pixels) return fail(SIFT_MI_EINVAL, "bad arguments");
    const uint8_t* frames[1] = {pixels};
    size_t offs[2];
    CHK(sift_mi_extract_batch(c, frames, 1, w, h, stride, limit, offs));
    if (n_keypoints) *n_keypoints = offs[1];
    return 0;
}

int sift_mi_fetch(sift_mi_ctx* c, sift_mi_keypoint* kps, uint8_t* desc, size_t cap) {
    if (!c) return fail(SIFT_MI_EINVAL, "ctx is null");
    if (!c->rs.can_fetch()) return fail(SIFT_MI_ESTATE, "no host result to fetch");
    const size_t n = c->rs.n;
    if (cap < n) return fail(SIFT_MI_EINVAL, "cap < result size");
    static_assert(sizeof(sift_mi_keypoint) == sizeof(OutKp), "layout");
    if (kps && n) par_memcpy(kps, c->h_kp.p, n * sizeof(OutKp));
    if (desc && n) par_memcpy(desc, c->h_desc.p, n * kDescSize);
    return 0;
}

int sift_mi_fetch_keys(sift_mi_ctx* c, uint64_t* keys, size_t cap) {
    if (!c || !keys) return fail(SIFT_MI_EINVAL, "bad arguments");
    if (!c->rs.can_fetch()) return fail(SIFT_MI_ESTATE, "no host result to fetch");
    if (cap < c->rs.n) return fail(SIFT_MI_EINVAL, "cap < result size");
    if (c->rs.n) par_memcpy(keys, c->h_key.p, c->rs.n * sizeof(uint64_t));
    return 0;
}

int sift_mi_device_results(sift_mi_ctx* c, const sift_mi_keypoint** d_kps, const uint8_t** d_desc, size_t* n) {
    if (!c) return fail(SIFT_MI_EINVAL, "ctx is null");
    if (!c->rs.can_device_results())
        return fail(SIFT_MI_ESTATE, c->rs.where == ResultWhere::host ? "the last result was copied to the host"
                                                                     : "no device result");
    const bool direct = c->res_slot >= 0;
    const Slot& S = c->slot[direct ? c->res_slot : 0];
    if (d_kps) *d_kps = reinterpret_cast<const sift_mi_keypoint*>(direct ? S.out_kp.p : c->r_kp.p);
    if (d_desc) *d_desc = direct ? S.out_desc.p : c->r_desc.p;
    if (n) *n = c->rs.n;
    return 0;
}

// ---- precompute_images / sift_with_precomputed (single frame) -------------
int sift_mi_precompute(sift_mi_ctx* c, const uint8_t* pixels, uint32_t w, uint32_t h, size_t stride,
                       size_t* n_octaves) {
    if (!c || !pixels) return fail(SIFT_MI_EINVAL, "bad arguments");
    CHK(check_frame_args(w, h, stride));
    CHK(set_device(c));
    const uint8_t* frames[1] = {pixels};
    CHK(upload_frames(c, frames, 1, w, h, stride));
    // the plan may be replaced and arena 0 is rewritten: an earlier pyramid, the
    // last batch's planes and the last result go, also when this call fails
    ProducingScope<> scope(c->rs);
    CHK(ensure_plan(c, w, h, 1));
    CHK(run_pyramid(c, 0, c->staging.p, (size_t)w * h, w, 1, true));
    HIPCHK(hipStreamSynchronize(c->stream));
    scope.done(ProducingCall::precompute, ResultWhere::none, 0, false);
    if (n_octaves) *n_octaves = (size_t)c->plan.n_oct;
    return 0;
}

int sift_mi_octave_dims(sift_mi_ctx* c, size_t o, uint32_t* w, uint32_t* h) {
    if (!c || !c->rs.can_read_pyramid()) return fail(SIFT_MI_ESTATE, "no precomputed pyramid");
    return octave_dims(c->plan, o, w, h);
}

int sift_mi_read_scale_space(sift_mi_ctx* c, size_t o, float* out) {
    if (!c || !out || !c->rs.can_read_pyramid()) return fail(SIFT_MI_ESTATE, "no precomputed pyramid");
    if (o >= (size_t)c->plan.n_oct) return fail(SIFT_MI_EINVAL, "octave out of range");
    CHK(set_device(c));
    return read_planes(c->plan, (int)o, c->plan.gauss((int)o), kImagesPerOctave, out);
}

int sift_mi_batch_octave_dims(sift_mi_ctx* c, size_t o, uint32_t* w, uint32_t* h) {
    if (!c || !c->rs.can_read_batch()) return fail(SIFT_MI_ESTATE, "no single-chunk batch pyramid");
    return octave_dims(c->plan, o, w, h);
}

int sift_mi_read_batch_scale_space(sift_mi_ctx* c, uint32_t frame, size_t o, float* out, size_t out_floats) {
    if (!c || !out || !c->rs.can_read_batch()) return fail(SIFT_MI_ESTATE, "no single-chunk batch pyramid");
    Plan& p = c->plan;
    if (o >= (size_t)p.n_oct || frame >= c->batch_frames || frame >= p.chunk)
        return fail(SIFT_MI_EINVAL, "frame / octave out of range");
    if (out_floats < (size_t)kImagesPerOctave * p.ow[o] * p.oh[o])
        return fail(SIFT_MI_EINVAL, "out_floats < 6 * width * height of the octave (sift_mi_batch_octave_dims)");
    CHK(set_device(c));
    CHK(sync_lanes(c));
    const float* g = p.gauss((int)o, c->batch_arena) + (size_t)frame * p.gstride((int)o);
    return read_planes(p, (int)o, g, kImagesPerOctave, out);
}

int sift_mi_read_dog(sift_mi_ctx* c, size_t o, float* out) {
    if (!c || !out || !c->rs.can_read_pyramid()) return fail(SIFT_MI_ESTATE, "no precomputed pyramid");
    if (o >= (size_t)c->plan.n_oct) return fail(SIFT_MI_EINVAL, "octave out of range");
    CHK(set_device(c));
    return read_planes(c->plan, (int)o, c->plan.dog((int)o), kDogPerOctave, out);
}

int sift_mi_sift_with_precomputed(sift_mi_ctx* c, int64_t limit, size_t* n_keypoints) {
    if (!c || !c->rs.can_begin(ProducingCall::with_precomputed)) return fail(SIFT_MI_ESTATE, "no precomputed pyramid");
    CHK(check_band_limit(c, limit));  // refused for its arguments: nothing changes
    CHK(set_device(c));
    // the stage and result buffers are rewritten (the planes are only read)
    ProducingScope<> scope(c->rs);
    c->call_dest = c->rs.destination(ProducingCall::with_precomputed);
    size_t offs[2];
    CHK(run_chunk_sync(c, nullptr, 0, 0, 1, limit, false, offs));
    scope.done(ProducingCall::with_precomputed, c->call_dest, offs[1], false);
    if (n_keypoints) *n_keypoints = offs[1];
    return 0;
}

// ---- compute_descriptor --------------------------------------------------
int sift_mi_compute_descriptor(sift_mi_ctx* c, const float* img, uint32_t w, uint32_t h, float x, float y,
                               float scale, float orientation, uint8_t* out) {
    if (!c || !img || !out || w < 1 || h < 1) return fail(SIFT_MI_EINVAL, "bad arguments");
    // window radius round(10.61 * scale) <= 39 (the device scratch); the
    // pipeline's keypoints have scale < 3.6 (radius <= 38)
    if (!(scale > 0.f) || roundf(3.0f * scale * 1.41421356f * 5.0f * 0.5f) > 39.0f)
        return fail(SIFT_MI_EUNSUPPORTED, "scale outside (0, 3.7]: descriptor window radius > 39");
    // the reference indexes its histogram out of bounds (panics) outside [0, 360]
    if (!(orientation >= 0.f && orientation <= 360.f)) return fail(SIFT_MI_EINVAL, "orientation outside [0, 360]");
    CHK(set_device(c));
    DevBuf<float> dimg;
    DevBuf<uint8_t> dout;
    CHK(upload(dimg, img, (size_t)w * h, c->stream));
    CHK(dout.ensure(kDescSize));
    launch_describe_one(dimg.p, (int)w, (int)h, x, y, scale, orientation, dout.p, c->stream);
    return download(out, dout, kDescSize, c->stream);
}

// ---- Processing ops ------------------------------------------------------
int sift_mi_gaussian_blur(sift_mi_ctx* c, const float* src, uint32_t w, uint32_t h, double sigma, float* dst) {
    if (!c || !src || !dst || w < 2 || h < 2 || !(sigma > 0)) return fail(SIFT_MI_EINVAL, "bad arguments");
    CHK(set_device(c));
    BlurTaps taps;
    const bool ip = c->profile == SIFT_MI_PROFILE_IMAGEPROC;
    const int r = ip ? ip_blur_taps((float)sigma, &taps) : cv_blur_taps(sigma, &taps);
    if (r < 1) return fail(SIFT_MI_EUNSUPPORTED, "blur radius outside 1..24");
    DevBuf<float> a, b;
    const size_t pitch = ((size_t)w + 63) & ~(size_t)63;  // same row alignment as the pyramid
    CHK(a.ensure(pitch * h));
    CHK(b.ensure(pitch * h));
    BlurLaunch L{};
    L.src = a.p;
    L.dst = b.p;
    L.W = (int)w;
    L.H = (int)h;
    L.pitch = (int)pitch;
    L.n_img = 1;
    L.taps = taps;
    L.profile = ip ? kProfileImageproc : kProfileOpenCV;
    if (hipMemcpy2DAsync(a.p, pitch * 4, src, (size_t)w * 4, (size_t)w * 4, h, hipMemcpyHostToDevice, c->stream) !=
            hipSuccess ||
        launch_blur(r, L, c->stream, c->opts) != 0 ||
        hipMemcpy2DAsync(dst, (size_t)w * 4, b.p, pitch * 4, (size_t)w * 4, h, hipMemcpyDeviceToHost, c->stream) !=
            hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(SIFT_MI_EHIP, "gaussian_blur failed");
    return 0;
}

int sift_mi_resize_linear(sift_mi_ctx* c, const float* src, uint32_t w, uint32_t h, uint32_t dw, uint32_t dh,
                          float* dst) {
    if (!c || !src || !dst || !w || !h || !dw || !dh) return fail(SIFT_MI_EINVAL, "bad arguments");
    CHK(set_device(c));
    if (c->profile == SIFT_MI_PROFILE_IMAGEPROC) return ip_resize_op(c, src, w, h, dw, dh, 1.0f, dst);
    ResizeTabDev tab;
    CHK(tab.upload((int)w, (int)h, (int)dw, (int)dh, c->stream));
    DevBuf<float> a, b;
    CHK(upload(a, src, (size_t)w * h, c->stream));
    CHK(b.ensure((size_t)dw * dh));
    launch_resize_linear_f32(a.p, (int)w, (int)h, tab.tab, b.p, (int)dw, (int)dh, c->stream);
    return download(dst, b, (size_t)dw * dh, c->stream);
}

int sift_mi_resize_nearest(sift_mi_ctx* c, const float* src, uint32_t w, uint32_t h, uint32_t dw, uint32_t dh,
                           float* dst) {
    if (!c || !src || !dst || !w || !h || !dw || !dh) return fail(SIFT_MI_EINVAL, "bad arguments");
    CHK(set_device(c));
    if (c->profile == SIFT_MI_PROFILE_IMAGEPROC) return ip_resize_op(c, src, w, h, dw, dh, 0.0f, dst);
    std::vector<int> xo, yo;
    cv_nearest_ofs((int)w, (int)dw, xo);
    cv_nearest_ofs((int)h, (int)dh, yo);
    DevBuf<float> a, b;
    DevBuf<int> dx, dy;
    CHK(upload(a, src, (size_t)w * h, c->stream));
    CHK(upload(dx, xo.data(), dw, c->stream));
    CHK(upload(dy, yo.data(), dh, c->stream));
    CHK(b.ensure((size_t)dw * dh));
    launch_resize_nearest_f32(a.p, (int)w, dx.p, dy.p, b.p, (int)dw, (int)dh, c->stream);
    return download(dst, b, (size_t)dw * dh, c->stream);
}

// ---- descriptor matching (examples/sift-match.rs:30-35) ---------------------
int sift_mi_match_descriptors(sift_mi_ctx* c, const uint8_t* query, size_t nq, const uint8_t* train, size_t nt,
                              int cross_check, sift_mi_match* out, size_t cap, size_t* n_matches) {
    if (!c || !n_matches || (nq && !query) || (nt && !train)) return fail(SIFT_MI_EINVAL, "bad arguments");
    if (nq > 0x7fffffff || nt > 0x7fffffff) return fail(SIFT_MI_EINVAL, "descriptor set too large");
    *n_matches = 0;
    if (nq == 0) return 0;
    CHK(set_device(c));
    DevBuf<uint8_t> dq, dt;
    DevBuf<float> qn, tn, dist;
    DevBuf<unsigned long long> rb, cb;
    DevBuf<int> tix;
    hipStream_t st = c->stream;
    CHK(upload(dq, query, nq * kDescSize, st));
    CHK(dt.ensure(std::max<size_t>(nt, 1) * kDescSize));
    if (nt) CHK(upload(dt, train, nt * kDescSize, st));
    CHK(qn.ensure(nq));
    CHK(tn.ensure(std::max<size_t>(nt, 1)));
    CHK(rb.ensure(nq));
    CHK(cb.ensure(std::max<size_t>(nt, 1)));
    CHK(tix.ensure(nq));
    CHK(dist.ensure(nq));
    std::vector<int> h_t(nq);
    std::vector<float> h_d(nq);
    launch_match(dq.p, (int)nq, dt.p, (int)nt, cross_check ? 1 : 0, qn.p, tn.p, rb.p, cb.p, tix.p, dist.p, st);
    HIPCHK(hipGetLastError());
    CHK(download(h_t.data(), tix, nq, st));
    CHK(download(h_d.data(), dist, nq, st));
    size_t n = 0;
    for (size_t i = 0; i < nq; i++) n += h_t[i] >= 0;
    *n_matches = n;
    if (cap < n || (n && !out)) return fail(SIFT_MI_EINVAL, "cap < number of matches");
    size_t k = 0;
    for (size_t i = 0; i < nq; i++)
        if (h_t[i] >= 0) out[k++] = sift_mi_match{(int32_t)i, h_t[i], h_d[i]};
    return 0;
}

// ---- 2-NN, ratio test, segment pairs (labelled extensions; match.hip) --------
int sift_mi_match_pairs_device(sift_mi_ctx* c, const uint8_t* d_desc, const size_t* offsets, uint32_t n_segs,
                               const sift_mi_seg_pair* pairs, uint32_t n_pairs, float ratio, int cross_check,
                               sift_mi_match* out, size_t cap, size_t* pair_offsets) {
    if (!c || !d_desc || !offsets || !pairs || !pair_offsets) return fail(SIFT_MI_EINVAL, "null argument");
    CHK(check_ratio(ratio));
    return match_guard([&]() -> int {
        std::vector<MatchPair> P;
        CHK(match_pairs_run(c, d_desc, offsets, n_segs, pairs, n_pairs, ratio, cross_check, false, P));
        return match_pairs_collect(c, P, out, cap, pair_offsets);
    });
}

int sift_mi_match_ratio(sift_mi_ctx* c, const uint8_t* query, size_t nq, const uint8_t* train, size_t nt,
                        float ratio, int cross_check, sift_mi_match* out, size_t cap, size_t* n_matches) {
    if (!c || !n_matches || (nq && !query) || (nt && !train)) return fail(SIFT_MI_EINVAL, "bad arguments");
    CHK(check_ratio(ratio));
    if (nq > 0x7fffffff || nt > 0x7fffffff || nq + nt > 0x7fffffff)
        return fail(SIFT_MI_EINVAL, "descriptor set too large");
    *n_matches = 0;
    if (nq == 0) return 0;
    return match_guard([&]() -> int {
        CHK(match_upload(c, query, nq, train, nt));
        const size_t offsets[3] = {0, nq, nq + nt};
        const sift_mi_seg_pair pair{0, 1};
        std::vector<MatchPair> P;
        CHK(match_pairs_run(c, c->match.desc.p, offsets, 2, &pair, 1, ratio, cross_check, false, P));
        size_t po[2] = {0, 0};
        const int rc = match_pairs_collect(c, P, out, cap, po);
        *n_matches = po[1];
        return rc;
    });
}

int sift_mi_match_neighbors(sift_mi_ctx* c, const uint8_t* query, size_t nq, const uint8_t* train, size_t nt,
                            sift_mi_neighbors* out) {
    if (!c || (nq && (!query || !out)) || (nt && !train)) return fail(SIFT_MI_EINVAL, "bad arguments");
    if (nq > 0x7fffffff || nt > 0x7fffffff || nq + nt > 0x7fffffff)
        return fail(SIFT_MI_EINVAL, "descriptor set too large");
    if (nq == 0) return 0;
    return match_guard([&]() -> int {
        CHK(match_upload(c, query, nq, train, nt));
        const size_t offsets[3] = {0, nq, nq + nt};
        const sift_mi_seg_pair pair{0, 1};
        std::vector<MatchPair> P;
        CHK(match_pairs_run(c, c->match.desc.p, offsets, 2, &pair, 1, 0.0f, 0, true, P));
        const int* idx = c->match.h_nb_idx.p;
        const float* dist = c->match.h_nb_dist.p;
        for (size_t i = 0; i < nq; i++)
            out[i] = sift_mi_neighbors{{idx[2 * i], idx[2 * i + 1]}, {dist[2 * i], dist[2 * i + 1]}};
        return 0;
    });
}

// ---- guided matching under verified models (labelled extension; match_guided.hip)
int sift_mi_match_pairs_guided_device(sift_mi_ctx* c, const uint8_t* d_desc, const sift_mi_keypoint* d_kps,
                                      const size_t* offsets, uint32_t n_segs, const sift_mi_seg_pair* pairs,
                                      uint32_t n_pairs, int model_kind, const float* models,
                                      const sift_mi_guided_params* params, sift_mi_match* out, size_t cap,
                                      size_t* pair_offsets) {
    if (!c || !d_desc || !d_kps || !offsets || !pairs || !models || !params || !pair_offsets)
        return fail(SIFT_MI_EINVAL, "null argument");
    return match_guard([&]() -> int {
        std::vector<MatchPair> P;
        CHK(match_guided_run(c, d_desc, reinterpret_cast<const OutKp*>(d_kps), offsets, n_segs, pairs, n_pairs,
                             model_kind, models, params, P));
        return match_pairs_collect(c, P, out, cap, pair_offsets);
    });
}

int sift_mi_match_guided(sift_mi_ctx* c, const uint8_t* query, const sift_mi_keypoint* query_kps, size_t nq,
                         const uint8_t* train, const sift_mi_keypoint* train_kps, size_t nt, int model_kind,
                         const float* model, const sift_mi_guided_params* params, sift_mi_match* out, size_t cap,
                         size_t* n_matches) {
    if (!c || !n_matches || !model || !params || (nq && (!query || !query_kps)) || (nt && (!train || !train_kps)))
        return fail(SIFT_MI_EINVAL, "null argument");
    if (nq > 0x7fffffff || nt > 0x7fffffff || nq + nt > 0x7fffffff)
        return fail(SIFT_MI_EINVAL, "descriptor set too large");
    *n_matches = 0;
    return match_guard([&]() -> int {
        CHK(check_guided(model_kind, params, model, 1));
        if (nq == 0) return 0;
        CHK(match_upload(c, query, nq, train, nt));
        const size_t offsets[3] = {0, nq, nq + nt};
        const sift_mi_seg_pair pair{0, 1};
        std::vector<MatchPair> P;
        CHK(match_guided_run(c, c->match.desc.p, nullptr, offsets, 2, &pair, 1, model_kind, model, params, P,
                             reinterpret_cast<const OutKp*>(query_kps), reinterpret_cast<const OutKp*>(train_kps)));
        size_t po[2] = {0, 0};
        const int rc = match_pairs_collect(c, P, out, cap, po);
        *n_matches = po[1];
        return rc;
    });
}

int sift_mi_guided_counters(sift_mi_ctx* c, uint64_t* tiles, uint64_t* culled_waves) {
    if (!c || !tiles || !culled_waves) return fail(SIFT_MI_EINVAL, "null argument");
    *tiles = c->match.guided_tiles;
    *culled_waves = c->match.guided_culled;
    return 0;
}

// ---- geometric verification (labelled extensions; verify.hip, verify_epipolar.hip)
namespace {
int verify_pairs_device(VerifyKind kind, sift_mi_ctx* c, const sift_mi_keypoint* d_kps, const size_t* offsets,
                        uint32_t n_segs, const sift_mi_seg_pair* pairs, uint32_t n_pairs, const sift_mi_match* matches,
                        const size_t* pair_offsets, const sift_mi_ransac_params* params, void* models,
                        uint8_t* inliers, VerifySampling sampling = VerifySampling::Uniform,
                        const float* quality = nullptr) {
    if (!c || !d_kps || !offsets || !pairs || !matches || !pair_offsets || !params || !models || !inliers)
        return fail(SIFT_MI_EINVAL, "null argument");
    return match_guard([&]() -> int {
        return verify_run(c, kind, reinterpret_cast<const OutKp*>(d_kps), offsets, n_segs, pairs, n_pairs, matches,
                          pair_offsets, params, models, inliers, nullptr, nullptr, sampling, quality);
    });
}

int verify_matches(VerifyKind kind, sift_mi_ctx* c, const sift_mi_keypoint* query_kps, size_t nq,
                   const sift_mi_keypoint* train_kps, size_t nt, const sift_mi_match* matches, size_t n_matches,
                   const sift_mi_ransac_params* params, void* model, uint8_t* inliers,
                   VerifySampling sampling = VerifySampling::Uniform, const float* quality = nullptr) {
    if (!c || !params || !model || (nq && !query_kps) || (nt && !train_kps) || (n_matches && (!matches || !inliers)))
        return fail(SIFT_MI_EINVAL, "null argument");
    if (nq > 0x7fffffff || nt > 0x7fffffff || nq + nt > 0x7fffffff)
        return fail(SIFT_MI_EINVAL, "keypoint set too large");
    return match_guard([&]() -> int {
        const size_t offsets[3] = {0, nq, nq + nt}, po[2] = {0, n_matches};
        const sift_mi_seg_pair pair{0, 1};
        return verify_run(c, kind, nullptr, offsets, 2, &pair, 1, matches, po, params, model, inliers,
                          reinterpret_cast<const OutKp*>(query_kps), reinterpret_cast<const OutKp*>(train_kps), sampling,
                          quality);
    });
}
}  // namespace

int sift_mi_verify_pairs_device(sift_mi_ctx* c, const sift_mi_keypoint* d_kps, const size_t* offsets, uint32_t n_segs,
                                const sift_mi_seg_pair* pairs, uint32_t n_pairs, const sift_mi_match* matches,
                                const size_t* pair_offsets, const sift_mi_ransac_params* params,
                                sift_mi_homography* models, uint8_t* inliers) {
    return verify_pairs_device(VerifyKind::Homography, c, d_kps, offsets, n_segs, pairs, n_pairs, matches, pair_offsets,
                               params, models, inliers);
}

int sift_mi_verify_matches(sift_mi_ctx* c, const sift_mi_keypoint* query_kps, size_t nq,
                           const sift_mi_keypoint* train_kps, size_t nt, const sift_mi_match* matches, size_t n_matches,
                           const sift_mi_ransac_params* params, sift_mi_homography* model, uint8_t* inliers) {
    return verify_matches(VerifyKind::Homography, c, query_kps, nq, train_kps, nt, matches, n_matches, params, model,
                          inliers);
}

int sift_mi_verify_pairs_epipolar_device(sift_mi_ctx* c, const sift_mi_keypoint* d_kps, const size_t* offsets,
                                         uint32_t n_segs, const sift_mi_seg_pair* pairs, uint32_t n_pairs,
                                         const sift_mi_match* matches, const size_t* pair_offsets,
                                         const sift_mi_ransac_params* params, sift_mi_fundamental* models,
                                         uint8_t* inliers) {
    return verify_pairs_device(VerifyKind::Fundamental, c, d_kps, offsets, n_segs, pairs, n_pairs, matches,
                               pair_offsets, params, models, inliers);
}

int sift_mi_verify_matches_epipolar(sift_mi_ctx* c, const sift_mi_keypoint* query_kps, size_t nq,
                                    const sift_mi_keypoint* train_kps, size_t nt, const sift_mi_match* matches,
                                    size_t n_matches, const sift_mi_ransac_params* params, sift_mi_fundamental* model,
                                    uint8_t* inliers) {
    return verify_matches(VerifyKind::Fundamental, c, query_kps, nq, train_kps, nt, matches, n_matches, params, model,
                          inliers);
}

// the same with progressive (PROSAC) sampling: prosac_growth.h, DESIGN.md 3.18
int sift_mi_verify_pairs_progressive_device(sift_mi_ctx* c, const sift_mi_keypoint* d_kps, const size_t* offsets,
                                            uint32_t n_segs, const sift_mi_seg_pair* pairs, uint32_t n_pairs,
                                            const sift_mi_match* matches, const size_t* pair_offsets,
                                            const float* quality, const sift_mi_ransac_params* params,
                                            sift_mi_homography* models, uint8_t* inliers) {
    return verify_pairs_device(VerifyKind::Homography, c, d_kps, offsets, n_segs, pairs, n_pairs, matches, pair_offsets,
                               params, models, inliers, VerifySampling::Progressive, quality);
}

int sift_mi_verify_matches_progressive(sift_mi_ctx* c, const sift_mi_keypoint* query_kps, size_t nq,
                                       const sift_mi_keypoint* train_kps, size_t nt, const sift_mi_match* matches,
                                       size_t n_matches, const float* quality, const sift_mi_ransac_params* params,
                                       sift_mi_homography* model, uint8_t* inliers) {
    return verify_matches(VerifyKind::Homography, c, query_kps, nq, train_kps, nt, matches, n_matches, params, model,
                          inliers, VerifySampling::Progressive, quality);
}

int sift_mi_verify_pairs_epipolar_progressive_device(sift_mi_ctx* c, const sift_mi_keypoint* d_kps,
                                                     const size_t* offsets, uint32_t n_segs,
                                                     const sift_mi_seg_pair* pairs, uint32_t n_pairs,
                                                     const sift_mi_match* matches, const size_t* pair_offsets,
                                                     const float* quality, const sift_mi_ransac_params* params,
                                                     sift_mi_fundamental* models, uint8_t* inliers) {
    return verify_pairs_device(VerifyKind::Fundamental, c, d_kps, offsets, n_segs, pairs, n_pairs, matches,
                               pair_offsets, params, models, inliers, VerifySampling::Progressive, quality);
}

int sift_mi_verify_matches_epipolar_progressive(sift_mi_ctx* c, const sift_mi_keypoint* query_kps, size_t nq,
                                                const sift_mi_keypoint* train_kps, size_t nt,
                                                const sift_mi_match* matches, size_t n_matches, const float* quality,
                                                const sift_mi_ransac_params* params, sift_mi_fundamental* model,
                                                uint8_t* inliers) {
    return verify_matches(VerifyKind::Fundamental, c, query_kps, nq, train_kps, nt, matches, n_matches, params, model,
                          inliers, VerifySampling::Progressive, quality);
}

// ---- feature tracks (labelled extension; tracks.hip) ---------------------------
int sift_mi_build_tracks_device(sift_mi_ctx* c, const sift_mi_keypoint* d_kps, const size_t* offsets, uint32_t n_segs,
                                const sift_mi_seg_pair* pairs, uint32_t n_pairs, const sift_mi_match* matches,
                                const size_t* pair_offsets, const uint8_t* keep, const sift_mi_track_params* params,
                                int32_t* track_of, uint32_t* n_tracks, uint32_t* track_offsets, sift_mi_track_obs* obs,
                                uint8_t* conflict) {
    if (!c || !d_kps || !offsets || !pairs || !matches || !pair_offsets || !params || !track_of || !n_tracks ||
        !track_offsets || !obs || !conflict)
        return fail(SIFT_MI_EINVAL, "null argument");
    return match_guard([&]() -> int {
        return tracks_run(c, reinterpret_cast<const OutKp*>(d_kps), offsets, n_segs, pairs, n_pairs, matches,
                          pair_offsets, keep, params, track_of, n_tracks, track_offsets, obs, conflict);
    });
}

int sift_mi_track_counters(sift_mi_ctx* c, double* kernel_ms, uint64_t* edges) {
    if (!c || !kernel_ms || !edges) return fail(SIFT_MI_EINVAL, "null argument");
    *kernel_ms = c->tracks.kernel_ms;
    *edges = c->tracks.edges;
    return 0;
}

// ---- frame-pair proposal (labelled extension; pairs.hip) -----------------------
int sift_mi_propose_pairs_device(sift_mi_ctx* c, const uint8_t* d_desc, const sift_mi_keypoint* d_kps,
                                 const size_t* offsets, uint32_t n_segs, const sift_mi_pair_params* params,
                                 uint32_t* scores, sift_mi_seg_pair* pairs, size_t cap, size_t* n_pairs) {
    if (!c || !d_desc || !d_kps || !offsets || !params || !pairs || !n_pairs)
        return fail(SIFT_MI_EINVAL, "null argument");
    *n_pairs = 0;
    return match_guard([&]() -> int {
        return pairs_run(c, d_desc, reinterpret_cast<const OutKp*>(d_kps), offsets, n_segs, params, scores, pairs, cap,
                         n_pairs);
    });
}

int sift_mi_pair_counters(sift_mi_ctx* c, double* kernel_ms, uint64_t* tiles) {
    if (!c || !kernel_ms || !tiles) return fail(SIFT_MI_EINVAL, "null argument");
    *kernel_ms = c->pairs.kernel_ms;
    *tiles = c->pairs.tiles;
    return 0;
}

// ---- spread-limited selection (labelled extension; select.hip) ------------------
int sift_mi_select_spread_device(sift_mi_ctx* c, const sift_mi_keypoint* d_kps, const uint8_t* d_desc,
                                 const size_t* offsets, uint32_t n_segs, const sift_mi_select_params* params,
                                 size_t* sel_offsets, uint32_t* rows, size_t cap, float* radius2) {
    if (!c || !d_kps || !offsets || !params || !sel_offsets || !rows) return fail(SIFT_MI_EINVAL, "null argument");
    return match_guard([&]() -> int {
        return select_run(c, reinterpret_cast<const OutKp*>(d_kps), nullptr, d_desc, offsets, n_segs, params,
                          sel_offsets, rows, cap, radius2);
    });
}

int sift_mi_selected_results(sift_mi_ctx* c, const sift_mi_keypoint** d_sel_kps, const uint8_t** d_sel_desc,
                             size_t* n) {
    if (!c || !d_sel_kps || !d_sel_desc || !n) return fail(SIFT_MI_EINVAL, "null argument");
    const SelectScratch& S = c->select;
    *d_sel_kps = reinterpret_cast<const sift_mi_keypoint*>(S.sel_kps.p);
    *d_sel_desc = S.has_desc ? S.sel_desc.p : nullptr;
    *n = S.n_sel;
    return 0;
}

int sift_mi_select_keypoints(sift_mi_ctx* c, const sift_mi_keypoint* kps, size_t n,
                             const sift_mi_select_params* params, uint32_t* rows, size_t cap, size_t* n_rows,
                             float* radius2) {
    if (!c || !kps || !params || !rows || !n_rows) return fail(SIFT_MI_EINVAL, "null argument");
    if (n > kSelectMaxRows) return fail(SIFT_MI_EINVAL, "keypoint set too large");
    return match_guard([&]() -> int {
        const size_t offsets[2] = {0, n};
        size_t sel[2] = {0, 0};
        const int rc = select_run(c, nullptr, reinterpret_cast<const OutKp*>(kps), nullptr, offsets, 1, params, sel,
                                  rows, cap, radius2);
        *n_rows = sel[1];
        return rc;
    });
}

int sift_mi_select_counters(sift_mi_ctx* c, double* kernel_ms, uint64_t* pair_tests) {
    if (!c || !kernel_ms || !pair_tests) return fail(SIFT_MI_EINVAL, "null argument");
    *kernel_ms = c->select.kernel_ms;
    *pair_tests = c->select.pair_tests;
    return 0;
}

int sift_mi_jpeg_dims(const uint8_t* data, size_t len, uint32_t* width, uint32_t* height) {
    if (!data || !width || !height) return fail(SIFT_MI_EINVAL, "bad arguments");
    return jpeg_guard([&]() -> int {
        std::string err;
        const int rc = jpeg_dims(data, len, width, height, err);
        return rc ? fail(rc, err) : 0;
    });
}

int sift_mi_decode_jpeg(sift_mi_ctx* c, const uint8_t* data, size_t len, uint8_t* out, size_t out_stride,
                        int out_on_device) {
    if (!c || !data || !out) return fail(SIFT_MI_EINVAL, "bad arguments");
    return jpeg_guard([&]() -> int {
        uint32_t w = 0, h = 0;
        std::string err;
        int rc = jpeg_dims(data, len, &w, &h, err);
        if (rc) return fail(rc, err);
        if (out_stride < w) return fail(SIFT_MI_EINVAL, "out_stride < width");
        CHK(set_device(c));
        rc = jpeg_decode_luma(data, len, out, out_stride, out_on_device != 0, c->stream, err);
        return rc ? fail(rc, err) : 0;
    });
}

int sift_mi_decode_jpeg_batch(sift_mi_ctx* c, const uint8_t* const* data, const size_t* len, uint32_t n,
                              uint8_t* d_frames, size_t frame_pitch, size_t row_stride, int threads) {
    if (!c || (n && (!data || !len || !d_frames))) return fail(SIFT_MI_EINVAL, "bad arguments");
    for (uint32_t i = 0; i < n; i++)
        if (!data[i]) return fail(SIFT_MI_EINVAL, "null JPEG");
    if (threads <= 0) threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    return jpeg_guard([&]() -> int {
    CHK(set_device(c));
    std::string err;
    // The reconstruction kernels run on a high-priority stream of their own
    // (ordered after the context's stream): the runtime takes its hardware
    // queue from the high-priority pool, so a decode pipelined beside another
    // context's batch (bench.py configs.jpeg_e2e) does not queue behind that
    // batch's kernels on a shared in-order queue -- normal-priority streams
    // share GPU_MAX_HW_QUEUES (4) queues round robin.  A caller stream
    // (sift_mi_set_stream) is used as is.  Measured (round 4), with the
    // polling host wait (host_wait_event): 2337 -> 3063 frames/s JPEG ->
    // keypoints, pipelined beside sift().
    hipStream_t st = c->stream;
    if (c->stream == c->own) {
        if (!c->dec) {
            int least = 0, greatest = 0;
            HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
            HIPCHK(hipStreamCreateWithPriority(&c->dec, hipStreamNonBlocking, greatest));
        }
        HIPCHK(hipEventRecord(c->fork, c->stream));
        HIPCHK(hipStreamWaitEvent(c->dec, c->fork, 0));
        st = c->dec;
    }
    const int rc = jpeg_decode_batch(data, len, n, d_frames, frame_pitch, row_stride, threads, st, c->jpeg, err);
    return rc ? fail(rc, err) : 0;
    });
}

int sift_mi_get_stats(sift_mi_ctx* c, sift_mi_stats* out) {
    if (!c || !out) return fail(SIFT_MI_EINVAL, "bad arguments");
    *out = c->stats;
    if (c->count_samples && c->samples.p) {
        CHK(set_device(c));
        CHK(sync_lanes(c));
        unsigned long long h[16];
        HIPCHK(hipMemcpy(h, c->samples.p, sizeof h, hipMemcpyDeviceToHost));
        out->orient_samples = out->desc_samples = 0;
        for (int i = 0; i < 8; i++) {
            out->orient_samples += h[i];
            out->desc_samples += h[8 + i];
        }
    }
    return 0;
}

int sift_mi_reset_stats(sift_mi_ctx* c) {
    if (!c) return fail(SIFT_MI_EINVAL, "ctx is null");
    c->stats = sift_mi_stats{};
    c->match.guided_tiles = c->match.guided_culled = 0;
    c->tracks.kernel_ms = 0;
    c->tracks.edges = 0;
    c->pairs.kernel_ms = 0;
    c->pairs.tiles = 0;
    c->select.kernel_ms = 0;
    c->select.pair_tests = 0;
    if (c->samples.p) {
        CHK(set_device(c));
        CHK(sync_lanes(c));
        HIPCHK(hipMemset(c->samples.p, 0, 16 * sizeof(unsigned long long)));
    }
    return 0;
}

int sift_mi_set_sample_counting(sift_mi_ctx* c, int on) {
    if (!c) return fail(SIFT_MI_EINVAL, "ctx is null");
    CHK(set_device(c));
    CHK(sync_lanes(c));
    if (on && !c->samples.p) {
        CHK(c->samples.ensure(16));
        HIPCHK(hipMemset(c->samples.p, 0, 16 * sizeof(unsigned long long)));
    }
    c->count_samples = on ? 1 : 0;
    return 0;
}

}  // extern "C"
