// libsift_mi.so host side: the pyramid plan and lanes, the pyramid's stream
// schedule (PyramidRun) and the chunk pipeline -- bounds, reserve, keypoint
// stages, finalize, overflow re-run, graph replay.  Mirrors the reference's
// pipeline (src/lib.rs:71-177): precompute_images -> find_keypoints -> [limit]
// -> compute_descriptors -> KeyPoint mapping, batched over equal-size frames.
#include <chrono>
#include <cmath>
#include <thread>

#include "host_internal.h"
#include "launch_ext.h"

namespace siftmi {

hipError_t host_wait_event(hipEvent_t e) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t r = hipEventQuery(e);
        if (r != hipErrorNotReady) return r;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(1000))
            std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

int IpTabDev::upload(int sw, int sh, int dw, int dh, float support, int min_taps, hipStream_t st) {
    auto axis = [&](int src, int dst, std::vector<int>& L, std::vector<float>& Wt, int& taps) {
        std::vector<std::vector<float>> ws(dst);
        L.resize(dst);
        taps = min_taps;
        std::vector<float> w(4096);
        for (int o = 0; o < dst; o++) {
            const int n = ip_axis(src, dst, o, support, &L[o], w.data());
            ws[o].assign(w.begin(), w.begin() + n);
            taps = std::max(taps, n);
        }
        Wt.assign((size_t)dst * taps, 0.0f);
        for (int o = 0; o < dst; o++)
            for (size_t k = 0; k < ws[o].size(); k++) Wt[(size_t)o * taps + k] = ws[o][k];
    };
    std::vector<int> lx, ly;
    std::vector<float> wx, wy;
    axis(sw, dw, lx, wx, xtaps);
    axis(sh, dh, ly, wy, ytaps);
    if (xtaps > 64 || ytaps > 64) return fail(SIFT_MI_EUNSUPPORTED, "resize ratio too large (> 64 taps)");
    CHK(siftmi::upload(xl, lx.data(), dw, st));
    CHK(siftmi::upload(yl, ly.data(), dh, st));
    CHK(siftmi::upload(xw, wx.data(), wx.size(), st));
    CHK(siftmi::upload(yw, wy.data(), wy.size(), st));
    HIPCHK(hipStreamSynchronize(st));  // host vectors go out of scope
    return 0;
}

int ResizeTabDev::upload(int sw, int sh, int dw, int dh, hipStream_t st) {
    std::vector<int> xo, yo;
    std::vector<float> xa, xb, ya, yb;
    int xmax = 0, ymax = 0;
    cv_linear_coeffs(sw, dw, xo, xa, xb, &xmax);
    cv_linear_coeffs(sh, dh, yo, ya, yb, &ymax);
    CHK(siftmi::upload(xofs, xo.data(), dw, st));
    CHK(siftmi::upload(xa0, xa.data(), dw, st));
    CHK(siftmi::upload(xa1, xb.data(), dw, st));
    CHK(siftmi::upload(yofs, yo.data(), dh, st));
    CHK(siftmi::upload(ya0, ya.data(), dh, st));
    CHK(siftmi::upload(ya1, yb.data(), dh, st));
    HIPCHK(hipStreamSynchronize(st));  // host vectors go out of scope
    tab = ResizeTab{xofs.p, xa0.p, xa1.p, yofs.p, ya0.p, ya1.p, xmax};
    return 0;
}

int sync_lanes(sift_mi_ctx* c) {
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipStreamSynchronize(c->own2));
    for (auto& a : c->aux) HIPCHK(hipStreamSynchronize(a));
    if (c->aux2) HIPCHK(hipStreamSynchronize(c->aux2));
    return 0;
}

int set_device(sift_mi_ctx* c) {
    HIPCHK(hipSetDevice(c->device));
    return 0;
}

int check_frame_args(uint32_t w, uint32_t h, size_t stride) {
    if (w < 1 || h < 1) return fail(SIFT_MI_EINVAL, "empty image");
    if (stride < w) return fail(SIFT_MI_EINVAL, "row_stride < width");
    if (w > kMaxFrameSide || h > kMaxFrameSide) return fail(SIFT_MI_EINVAL, "image larger than 16384 px (key field)");
    return 0;
}

int upload_frames(sift_mi_ctx* c, const uint8_t* const* frames, uint32_t n, uint32_t w, uint32_t h, size_t stride) {
    const size_t pitch = (size_t)w * h;
    CHK(c->staging.ensure(pitch * n));
    for (uint32_t i = 0; i < n; i++) {
        if (!frames[i]) return fail(SIFT_MI_EINVAL, "null frame");
        HIPCHK(hipMemcpy2DAsync(c->staging.p + i * pitch, w, frames[i], stride, w, h, hipMemcpyHostToDevice,
                                c->stream));
    }
    return 0;
}

namespace {

// slot si's stream and pyramid arena: its own lane with two lanes, else lane 0
hipStream_t lane_stream(sift_mi_ctx* c, int si) { return (si == 1 && c->lanes == 2) ? c->own2 : c->stream; }
int arena_of(const sift_mi_ctx* c, int si) { return c->lanes == 2 ? si : 0; }

// completion events carried by kernel launches: not under stream capture (a
// kernel's stop event does not become a graph dependency, so captured work
// would not wait for it)
bool launch_events_allowed(hipStream_t st) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone;
}

// Pyramid arena of one pipeline lane (chunks alternate between two lanes so
// that one chunk's kernels overlap the other's) and its device pointer table.
int ensure_lane(sift_mi_ctx* c, int lane) {
    Plan& p = c->plan;
    if (p.arena[lane].p && p.d_gauss[lane].p) return 0;
    CHK(p.arena[lane].ensure(p.arena_floats));
    std::vector<const float*> gp(p.n_oct);
    for (int o = 0; o < p.n_oct; o++) gp[o] = p.gauss(o, lane);
    CHK(upload(p.d_gauss[lane], gp.data(), p.n_oct, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// ---------------------------------------------------------------------------
// Stages 2-4 for the m frames in the pyramid arena: detection, refinement,
// orientation, ordering, features_limit, descriptors -- enqueued on the
// compute stream with no host round trip.  Every stage reads its input count
// from device memory (Slot::counters) and is bounded by a host-side estimate
// (bc / be / bk); finalize_chunk detects a count above its bound and the chunk
// is re-run with larger bounds.
// ---------------------------------------------------------------------------
struct Bounds {
    uint32_t bc, be, bk;
};

Bounds chunk_bounds(sift_mi_ctx* c, uint32_t m) {
    const uint64_t sum_p = c->plan.sum_px;
    auto est = [&](double pf, double floor_pf) {
        const double per = std::max(pf * 1.3, floor_pf);
        return (uint32_t)std::min<double>(std::ceil(per * m) + 1024, 0x7fffffff);
    };
    Bounds B;
    // first chunk: one candidate per 256 octave pixels; later chunks: 1.3x
    // the per-frame high-water mark.  PathOpts::bound_shrink = k (test path)
    // divides the first-chunk estimates by k and drops the slack, so every
    // chunk enqueued before a high-water mark exists overflows and re-runs.
    const double shrink = std::max(1, c->opts.bound_shrink);
    if (shrink > 1.0 && c->pf_cand == 0) {
        auto tiny = [&](double per) { return (uint32_t)std::max(1.0, std::ceil(per / shrink * m)); };
        B.bc = tiny(sum_p / 256.0);
        B.be = std::min(B.bc, tiny(sum_p / 512.0));
        B.bk = tiny(sum_p / 384.0);
        return B;
    }
    B.bc = est(c->pf_cand, c->pf_cand > 0 ? 64.0 : sum_p / 256.0);
    B.be = est(c->pf_ext, c->pf_ext > 0 ? 64.0 : sum_p / 512.0);
    B.bk = est(c->pf_kp, c->pf_kp > 0 ? 64.0 : sum_p / 384.0);
    B.be = std::min(B.be, B.bc);  // one extremum per candidate at most
    return B;
}

// Grows the shared buffers for bounds B (waits for in-flight work first when a
// buffer has to be reallocated).
// frames: the slot's frame capacity (the plan's chunk); m: this chunk's frames
int reserve_chunk(sift_mi_ctx* c, int si, const Bounds& B, uint32_t frames, uint32_t m) {
    Slot& S = c->slot[si];
    const CounterLayout L{frames};
    // the tail octaves' own candidate / extremum region (Slot::early): a
    // 1.3x per-frame high-water mark, at least 2048
    const uint32_t bcb =
        std::max<uint32_t>(2048, (uint32_t)std::min<double>(std::ceil(c->pf_cand_b * 1.3 * frames) + 1024, 1e9));
    const bool grow = B.bc > S.cand.cap || B.be > S.ext.cap || B.bk > S.kp.cap || B.bk > S.keys_a.cap ||
                      bcb > S.cand_b.cap || bcb > S.ext_b.cap ||
                      frames > S.seg_off.cap || B.bk > S.out_kp.cap ||
                      L.device_words() > S.counters.cap ||
                      (m == 1 && (size_t)B.bk * kDescSize > S.desc_kp.cap);
    if (grow) {
        HIPCHK(hipStreamSynchronize(lane_stream(c, si)));
        HIPCHK(hipStreamSynchronize(c->cstream));
        if (si == 0 && c->lanes == 2) HIPCHK(hipStreamSynchronize(c->own2));  // one-chunk calls' second stream
    }
    CHK(S.cand.ensure(B.bc));
    CHK(S.ext.ensure(B.be));
    S.bcb = bcb;
    CHK(S.cand_b.ensure(S.bcb));
    CHK(S.ext_b.ensure(S.bcb));
    CHK(S.kp.ensure(B.bk));
    CHK(S.keys_a.ensure(B.bk));
    CHK(S.keys_b.ensure(B.bk));
    CHK(S.vals_a.ensure(B.bk));
    CHK(S.vals_b.ensure(B.bk));
    CHK(S.fin.ensure(B.bk));
    CHK(S.seg_off.ensure(frames));
    CHK(S.out_off.ensure(frames));
    CHK(S.use_resp.ensure(frames));
    CHK(S.counters.ensure(L.device_words()));
    CHK(S.h_counts.ensure(L.host_words()));
    CHK(S.out_kp.ensure(B.bk));
    CHK(S.out_desc.ensure((size_t)B.bk * kDescSize));
    CHK(S.out_key.ensure(B.bk));
    if (m == 1) CHK(S.desc_kp.ensure((size_t)B.bk * kDescSize));  // Slot::desc_first
    return 0;
}

int img_bits_for(uint32_t m) {
    int b = 1;
    while ((1u << b) <= m) b++;  // strictly above the largest frame index: the padding key sorts last
    return b;
}

// Zeroed counters of slot si (stage counts, frame starts = ~0, tail region,
// descriptor work queues), before any of its kernels that count.
void flush_chunk_init(sift_mi_ctx* c, int si) {
    Slot& S = c->slot[si];
    if (!S.init_pending) return;
    S.init_pending = false;
    launch_chunk_init(S.counters.p, (int)S.m, (int)S.layout().reset_words(), lane_stream(c, si));
}

// The host-side state of a chunk about to be enqueued on slot S
// (finalize_chunk reads it).
void set_chunk_state(Slot& S, uint32_t m, uint32_t frame_base, const Bounds& B) {
    S.m = m;
    S.frame_base = frame_base;
    S.bc = B.bc;
    S.be = B.be;
    S.bk = B.bk;
    S.detected = false;
    S.fused_mask = 0;
    S.graph_run = false;
    S.early = false;
    S.join_pending = false;
}

// Per-chunk state and zeroed counters of slot si, before any of its kernels
// (detection may start inside the pyramid: stage overlap).
int prepare_chunk(sift_mi_ctx* c, int si, uint32_t m, uint32_t frame_base, const Bounds& B, bool defer_init) {
    set_chunk_state(c->slot[si], m, frame_base, B);
    c->slot[si].init_pending = true;
    if (!defer_init) flush_chunk_init(c, si);
    HIPCHK(hipGetLastError());
    return 0;
}

// Detection of octaves [o0, o1) of frames [f0, f0 + nf) of slot si's chunk:
// one multi-octave k_detect_rows launch (candidates into the slot's buffer,
// bounded by S.bc).
int launch_detection(sift_mi_ctx* c, int si, uint32_t f0, uint32_t nf, int o0, int o1, hipStream_t st,
                     uint64_t* cand = nullptr, uint32_t* counter = nullptr, uint32_t cap = 0) {
    Plan& p = c->plan;
    Slot& S = c->slot[si];
    DetectLaunch D{};
    D.n_img = (int)nf;
    D.img_base = (int)f0;  // frame index within the chunk (emission keys)
    D.cand = cand ? cand : S.cand.p;
    D.counter = cand ? counter : S.counters.p + S.layout().cand();
    D.cap = cand ? cap : S.bc;
    int k = 0;
    for (int o = o0; o < o1; o++) {
        if (p.oh[o] < 2 * kImageBorder || p.ow[o] < 2 * kImageBorder) continue;  // src/lib.rs:315
        if ((S.fused_mask >> o) & 1) continue;  // detected with its blur 5 (k_blur_detect)
        DetectOctave& d = D.oct[k++];
        d.gauss = p.gauss(o, arena_of(c, si)) + (size_t)f0 * p.gstride(o);
        d.img_stride = p.gstride(o);
        d.W = p.ow[o];
        d.H = p.oh[o];
        d.pitch = p.opitch[o];
        d.octave = o;
        // row band: octave rows [H*r/n, H*(r+1)/n) -- the bands of one
        // octave partition its rows, so every candidate (keyed by its
        // initial octave, scale, y, x) belongs to exactly one band
        d.y_lo = band_row_lo(p.oh[o], c->band_r, c->band_n);
        d.y_hi = band_row_hi(p.oh[o], c->band_r, c->band_n);
    }
    D.n_oct = k;
    if (k) launch_detect(D, st);
    S.detected = true;
    HIPCHK(hipGetLastError());
    return 0;
}

// refinement of the candidates (cand, *n_cand <= cand_cap) into ext (*counter,
// cap), and orientation of those extrema into the slot's keypoints
// (counter_hi / n_ext_hi: two-ended extremum append, RefineLaunch::counter_hi)
int launch_refine_stage(sift_mi_ctx* c, int si, const uint64_t* cand, const uint32_t* n_cand, uint32_t cand_cap,
                        ExtRec* ext, uint32_t* counter, uint32_t cap, hipStream_t st,
                        uint32_t* counter_hi = nullptr) {
    RefineLaunch R{};
    R.counter_hi = counter_hi;
    R.cand = cand;
    R.n_cand = n_cand;
    R.cand_cap = cand_cap;
    R.band_flag = c->band_restricted ? c->band_flag.p : nullptr;
    R.band_r = (int)c->band_r;
    R.band_n = (int)c->band_n;
    R.band_patch = kBandPatch;
    // kBandDrift + 1 + kBandPatch; PathOpts::band_drift narrows the rows the
    // check accepts (down to -kBandPatch: patches may not cross the band
    // edge; tests force the re-run path)
    R.band_margin = kBandPatch + 1 + std::min(kBandDrift, std::max(-kBandPatch, c->opts.band_drift));
    R.oct = c->plan.view(arena_of(c, si));
    R.n_oct = c->plan.n_oct;
    R.img_base = 0;
    R.out = ext;
    R.counter = counter;
    R.cap = cap;
    launch_refine(R, st);
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_orient_stage(sift_mi_ctx* c, int si, const ExtRec* ext, const uint32_t* n_ext, uint32_t ext_cap,
                        uint32_t kp_cap, hipStream_t st, const uint32_t* n_ext_hi = nullptr) {
    Slot& S = c->slot[si];
    OrientLaunch O{};
    O.ext = ext;
    O.n_ext_hi = n_ext_hi;
    O.n_ext = n_ext;
    O.ext_cap = ext_cap;
    O.oct = c->plan.view(arena_of(c, si));
    O.out = S.kp.p;
    O.counter = S.counters.p + S.layout().kp();
    O.img_base = 0;
    O.cap = kp_cap;
    O.samples = c->count_samples ? c->samples.p : nullptr;
    launch_orient(O, st);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// Stage 1: Gaussian scale space + DoG for n frames (device-resident u8)
// ---------------------------------------------------------------------------
// full: materialise every image (precompute_images / read_dog); the batch
// path writes G_0..G_5 only: detection and refinement form D_s = G_{s+1} - G_s
// where they read it (detect.hip), 16 B per octave pixel less than writing
// the DoG planes and reading them back.
// Octave overlap: octave o + 1 needs only G_3 of octave o (its G_0 is
// written by blur 3), so blurs 4, 5 of each octave run on the lane's aux
// stream beside the next octave's blurs (without: 0.779 vs 0.62 ms per 1080p
// frame, round 4).  Tried and measured slower or no faster (round 3, DESIGN.md
// 3.10): the chunk's
// frames split in two halves on the two streams; seed + octave 0 in
// sub-batches of 2-32 frames for Infinity Cache reuse; a second aux stream;
// only octaves 0 .. k-1 (k = 1, 2, 3) on the aux stream.
// detect_slot >= 0 (stage overlap): the detection of the chunk in that slot
// is launched from here, each part's octaves as soon as their blurs are done.
// cand_slot >= 0 (the keypoint stages follow): octaves whose blur 5 and
// detection run as one pass (k_blur_detect) append their candidates to that
// slot's buffer from here, whatever detect_slot is (Slot::fused_mask).
//
// One run_pyramid call: its inputs, what run_pyramid derives from them, and
// the state its launches hand to one another.
struct PyramidRun {
    sift_mi_ctx* c;
    Plan& p;
    const PathOpts& po;
    int lane;  // the arena
    hipStream_t aux, aux2;
    const uint8_t* d_frames;
    size_t frame_pitch, row_stride;
    bool full;
    int detect_slot, cand_slot;  // cand_slot: the chunk's slot
    // row bands (sift_mi_set_row_band): the rows of every Gaussian this
    // band's keypoint stages read (band_rows).  A refinement that reads, or
    // an accepted keypoint whose patch reaches, beyond them sets band_flag
    // (k_refine) and the host re-runs the band on the whole pyramid.
    BandRows rows;
    int seed_y0 = 0, seed_y1 = 0;
    // the small octaves from o_tail on: one k_octave_tail launch
    // (PathOpts::tail = 0: per-blur launches for every octave)
    int o_tail;
    // the launch that writes an octave's G_3 signals the aux stream's event
    // itself: no marker packet on the main stream (a separate event record
    // after it: 0.626 / 0.629 vs 0.616 / 0.619 ms per 1080p frame, round 4)
    bool ext_events;
    // the seed and blur 1 ran as one pass (k_seed_pair): octave 0 continues
    // at blur 2, as the (2, 3) pair
    bool seed_pair = false;
    // Octave 0's fused blur 5 + scan (k_blur_detect, the stage's longest
    // launch) is deferred until octave 1's G_3 is written, and the blurs 4, 5
    // of octaves >= 1 go to a second aux stream: octave 1's blur 3 then does
    // not run starved beside it (round 4: 3.4 ms at 0.35 TB/s), and the small
    // octaves' chain runs beside the long pass instead of after it.
    bool defer0 = false;  // octave 0's blur 5 is pending (deferral)
    BlurDetectLaunch defer_f{};
    bool used_aux2 = false;
    uint64_t launches = 0;

    int row_lo(int o, int s) const { return rows.lo[(size_t)o * kImagesPerOctave + s]; }
    int row_hi(int o, int s) const { return rows.hi[(size_t)o * kImagesPerOctave + s]; }

    // blur s of octave o for frames [f0, f0 + nf)
    BlurLaunch blur_launch(int o, int s, uint32_t f0, uint32_t nf) const {
        float* G = p.gauss(o, lane) + (size_t)f0 * p.gstride(o);
        const size_t P = p.P[o];
        BlurLaunch B{};
        B.src = G + (size_t)(s - 1) * P;
        B.src_img_stride = p.gstride(o);
        B.dst = G + (size_t)s * P;
        B.dst_img_stride = p.gstride(o);
        if (s == 3 && o + 1 < p.n_oct) {
            B.nxt = p.gauss(o + 1, lane) + (size_t)f0 * p.gstride(o + 1);
            B.nxt_img_stride = p.gstride(o + 1);
            B.pitch_n = p.opitch[o + 1];
            B.wn = p.ow[o + 1];
            B.hn = p.oh[o + 1];
        }
        B.W = p.ow[o];
        B.H = p.oh[o];
        B.pitch = p.opitch[o];
        B.n_img = (int)nf;
        B.taps = p.oct_taps[s];
        B.profile = p.profile;
        if (c->band_restricted) {
            B.y0 = row_lo(o, s);
            B.y1 = std::max(row_hi(o, s), B.y0 + 1);
        }
        return B;
    }

    // the seed of frames [f0, f0 + nf) on stream sm
    int seed(uint32_t f0, uint32_t nf, hipStream_t sm) {
        SeedLaunch S{};
        S.frames = d_frames + (size_t)f0 * frame_pitch;
        S.frame_pitch = frame_pitch;
        S.row_stride = row_stride;
        S.sh = (int)p.h;
        S.sw = (int)p.w;
        S.tab = p.seed_tab.tab;
        S.iptab = p.seed_iptab.tab();
        S.profile = p.profile;
        S.dst = p.gauss(0, lane) + (size_t)f0 * p.gstride(0);
        S.dst_img_stride = p.gstride(0);
        S.W = p.ow[0];
        S.H = p.oh[0];
        S.pitch = p.opitch[0];
        S.n_img = (int)nf;
        S.taps = p.seed_taps;
        S.y0 = seed_y0;
        S.y1 = seed_y1;
        // the chunk's counter reset rides on the seed pass (its first workgroup)
        Slot* is = (cand_slot >= 0 && f0 == 0 && c->slot[cand_slot].init_pending) ? &c->slot[cand_slot] : nullptr;
        if (is) {
            S.init_cnt = is->counters.p;
            S.init_m = (int)is->m;
            S.init_words = (int)is->layout().reset_words();
        }
        // G_0 and G_1 in one pass where it applies (whole planes: not for a
        // restricted row band); G_0 is then never read back from HBM
        seed_pair = p.n_oct > 0 && launch_seed_pair(p.seed_r, p.oct_r[1], S, blur_launch(0, 1, f0, nf), sm, po) == 0;
        if (seed_pair && is) is->init_pending = false;
        if (!seed_pair && launch_seed(p.seed_r, S, sm, po)) return fail(SIFT_MI_EUNSUPPORTED, "seed blur radius");
        launches++;
        return 0;
    }

    // octave 0's deferred fused pass, on the aux stream once oct_ev[lane][o] is done
    int launch_deferred(int o) {
        HIPCHK(hipStreamWaitEvent(aux, c->oct_ev[lane][o], 0));
        if (launch_blur_detect(p.oct_r[5], defer_f, aux, po) != 0)
            return fail(SIFT_MI_EHIP, "deferred blur-detect launch declined");
        defer0 = false;
        return 0;
    }

    // octaves [o0, o1) of frames [f0, f0 + nf) on stream sm; ov: blurs 4, 5 of
    // each octave on the aux stream
    int octaves(uint32_t f0, uint32_t nf, int o0, int o1, hipStream_t sm, bool ov) {
        hipStream_t s45 = sm;
        for (int o = o0; o < o1; o++) {
            bool g3_signalled = false;
            float* G = p.gauss(o, lane) + (size_t)f0 * p.gstride(o);
            // octave 0 after k_seed_pair starts at blur 2
            for (int s = (o == 0 && seed_pair) ? 2 : 1; s < kImagesPerOctave; s++) {
                if (s == 4 && ov) {
                    if (!g3_signalled) HIPCHK(hipEventRecord(c->oct_ev[lane][o], sm));
                    // octave 1's G_3 is on its way: octave 0's fused pass
                    // now, the octaves from here on on the second aux stream
                    if (o >= 1 && defer0) CHK(launch_deferred(o));
                    hipStream_t a = (o >= 1 && used_aux2) ? aux2 : aux;
                    HIPCHK(hipStreamWaitEvent(a, c->oct_ev[lane][o], 0));
                    s45 = a;
                }
                const BlurLaunch B = blur_launch(o, s, f0, nf);
                // blur 5 and the octave's detection in one pass (k_blur_detect:
                // G_4 / G_5 never read back by the extremum scan)
                if (s == kImagesPerOctave - 1 && cand_slot >= 0 && !full && c->band_n <= 1 && o < 32) {
                    Slot& S = c->slot[cand_slot];
                    BlurDetectLaunch F{};
                    F.gauss = G;
                    F.img_stride = p.gstride(o);
                    F.W = p.ow[o];
                    F.H = p.oh[o];
                    F.pitch = p.opitch[o];
                    F.octave = o;
                    F.n_img = (int)nf;
                    F.img_base = (int)f0;
                    F.profile = p.profile;
                    F.taps = p.oct_taps[s];
                    F.cand = S.cand.p;
                    F.counter = S.counters.p + S.layout().cand();
                    F.cap = S.bc;
                    // defer octave 0's pass (see above) when it is fused and a
                    // later octave will take the second aux stream
                    if (o == 0 && ov && aux2 && o1 > 1 && blur_detect_applies(p.oct_r[s], F, po)) {
                        defer_f = F;
                        defer0 = true;
                        used_aux2 = true;
                        S.fused_mask |= 1u << o;
                        launches++;
                        continue;
                    }
                    if (launch_blur_detect(p.oct_r[s], F, s45, po) == 0) {
                        S.fused_mask |= 1u << o;
                        launches++;
                        continue;
                    }
                }
                // G_1, G_2 in one pass where the pair kernel applies
                // (k_blur2_strip: G_1 never read back from HBM); after the
                // seed pair, G_2, G_3 (and the next octave's base) instead.
                // g3: this launch writes G_3 (blur 3, or the octave-0 (2, 3)
                // pair) and carries the aux stream's event.
                const bool pair = s == 1 || (s == 2 && o == 0 && seed_pair);
                const bool g3 = ov && ext_events && (s == 3 || (s == 2 && o == 0 && seed_pair));
                if (pair) {
                    LaunchDoneEvent done(g3 ? c->oct_ev[lane][o] : nullptr);
                    if (launch_blur_pair(p.oct_r[s], p.oct_r[s + 1], B, blur_launch(o, s + 1, f0, nf), sm, po) == 0) {
                        g3_signalled = done.taken();
                        launches++;
                        s++;
                        continue;
                    }
                    // a declined pair launched nothing; blur s alone does not
                    // write G_3, so it goes out without the event and blur 3
                    // arms its own
                }
                LaunchDoneEvent done(g3 && s == 3 ? c->oct_ev[lane][o] : nullptr);
                if (launch_blur(p.oct_r[s], B, s >= 4 ? s45 : sm, po))
                    return fail(SIFT_MI_EUNSUPPORTED, "octave blur radius");
                g3_signalled = g3_signalled || done.taken();
                launches++;
            }
            // precompute_images: D_s = G_{s+1} - G_s, the same f32 subtraction
            // the keypoint stages form where they read the DoG
            if (full) dog(o, f0, nf, s45);
        }
        return 0;
    }

    // one frame's D (octave_geometry) of a `full` run
    void dog(int o, uint32_t f0, uint32_t nf, hipStream_t sm) {
        launch_dog(p.gauss(o, lane) + (size_t)f0 * p.gstride(o), p.P[o], p.gstride(o),
                   p.dog(o, lane) + (size_t)f0 * p.dstride(o), p.dstride(o), p.ow[o], p.oh[o], p.opitch[o], (int)nf,
                   sm);
    }

    // frames [f0, f0 + nf): seed, octave chain, tail (and their detection) on
    // stream sm; ov: blurs 4, 5 of each octave on the aux stream
    int part(uint32_t f0, uint32_t nf, hipStream_t sm, bool ov) {
        bool aux_done_signalled = false;  // the aux orientation's launch carries the join event
        const bool early =
            detect_slot >= 0 && ov && o_tail > 0 && o_tail < p.n_oct && c->slot[detect_slot].bcb && po.early;
        CHK(seed(f0, nf, sm));
        if (cand_slot >= 0 && f0 == 0) flush_chunk_init(c, cand_slot);  // the chunk's counters, behind the seed
        CHK(octaves(f0, nf, 0, o_tail, sm, ov));
        // no later octave took it (cannot happen with o_tail > 1): launch it now
        if (defer0) CHK(launch_deferred(0));
        if (used_aux2) {  // the aux stream's later work (detection, join) follows the second's
            HIPCHK(hipEventRecord(c->aux2_join, aux2));
            HIPCHK(hipStreamWaitEvent(aux, c->aux2_join, 0));
        }
        if (o_tail < p.n_oct) {
            // whole octaves (a row band's restricted rows are a subset: rows
            // outside them depend only on rows outside them, so the exact rows
            // stay exact)
            TailLaunch T{};
            for (int o = 0; o < p.n_oct; o++) {
                T.gauss[o] = p.gauss(o, lane) + (size_t)f0 * p.gstride(o);
                T.gstride[o] = p.gstride(o);
                T.ow[o] = p.ow[o];
                T.oh[o] = p.oh[o];
                T.pitch[o] = p.opitch[o];
            }
            T.o0 = o_tail;
            T.n_oct = p.n_oct;
            T.n_img = (int)nf;
            T.profile = p.profile;
            for (int s = 1; s < kImagesPerOctave; s++) {
                T.r[s] = p.oct_r[s];
                T.taps[s] = p.oct_taps[s];
            }
            launch_octave_tail(T, sm);
            launches++;
            if (full)
                for (int o = o_tail; o < p.n_oct; o++) dog(o, f0, nf, sm);
        }
        if (early) {
            // one chunk (octave overlap): the octaves below the tail are
            // detected, refined and oriented on the aux stream beside the tail
            // kernel; the tail octaves, after it, into a region of their own
            // (Slot::early; PathOpts::early = 0: off).  Tried and dropped: the
            // large octaves detected on lane 1's stream as each one's G_5
            // lands (0.634 vs 0.613-0.624 ms per 1080p frame: the scan then
            // competes with the blur chain for HBM instead of filling the
            // idle chip beside the one-workgroup tail kernel)
            Slot& S = c->slot[detect_slot];
            const CounterLayout L = S.layout();
            uint32_t* cnt = S.counters.p;
            CHK(launch_detection(c, detect_slot, f0, nf, 0, o_tail, aux));
            // (PathOpts::large_first: two-ended extremum append, large
            // descriptor windows first)
            uint32_t* ext_hi = po.large_first ? cnt + L.ext_back() : nullptr;
            CHK(launch_refine_stage(c, detect_slot, S.cand.p, cnt + L.cand(), S.bc, S.ext.p, cnt + L.ext(), S.be, aux,
                                    ext_hi));
            {
                // the aux orientation signals the join event itself (no marker
                // on the aux stream's critical path; not under stream capture)
                LaunchDoneEvent done(ext_events ? c->oct_ev[lane][kTailMaxOct] : nullptr);
                CHK(launch_orient_stage(c, detect_slot, S.ext.p, cnt + L.ext(), S.be, S.bk, aux, ext_hi));
                aux_done_signalled = done.taken();
            }
            CHK(launch_detection(c, detect_slot, f0, nf, o_tail, p.n_oct, sm, S.cand_b.p, cnt + L.tail_cand(), S.bcb));
            CHK(launch_refine_stage(c, detect_slot, S.cand_b.p, cnt + L.tail_cand(), S.bcb, S.ext_b.p,
                                    cnt + L.tail_ext(), S.bcb, sm));
            CHK(launch_orient_stage(c, detect_slot, S.ext_b.p, cnt + L.tail_ext(), S.bcb, S.bk, sm));
            S.early = true;
        } else if (detect_slot >= 0) {
            // octaves [0, o_tail) are complete once their last blur is done:
            // with ov their detection runs on the aux stream beside the tail
            CHK(launch_detection(c, detect_slot, f0, nf, 0, o_tail, ov && o_tail > 0 ? aux : sm));
            CHK(launch_detection(c, detect_slot, f0, nf, o_tail, p.n_oct, sm));
        }
        if (ov && o_tail > 0) {  // join: the aux stream's work before what follows on sm
            if (!aux_done_signalled) HIPCHK(hipEventRecord(c->oct_ev[lane][kTailMaxOct], aux));
            // (not under stream capture: a capture keeps the plain join)
            if (early && c->lanes == 2 && ext_events)
                c->slot[detect_slot].join_pending = true;  // enqueue_keypoints joins
            else
                HIPCHK(hipStreamWaitEvent(sm, c->oct_ev[lane][kTailMaxOct], 0));
        }
        return 0;
    }
};

int enqueue_keypoints(sift_mi_ctx* c, int si, uint32_t m, int64_t limit, uint32_t frame_base, const Bounds& B) {
    Plan& p = c->plan;
    Slot& S = c->slot[si];
    hipStream_t st = lane_stream(c, si);
    const CounterLayout L = S.layout();
    uint32_t* cnt = S.counters.p;
    uint32_t* n_kp = cnt + L.kp();
    uint32_t* n_out = cnt + L.out();
    uint32_t* starts = cnt + L.starts();
    // one frame, no limit, early detection: the descriptors are computed in
    // keypoint index order beside the ordering stage, which runs on lane 1's
    // idle stream; k_gather_out then writes the outputs in emission order
    // (PathOpts::desc_first = 0: order, then describe in emission order)
    S.desc_first = S.early && m == 1 && limit < 0 && si == 0 && c->lanes == 2 &&
                   S.desc_kp.cap >= (size_t)B.bk * kDescSize && c->opts.desc_first;
    const bool join_pending = S.join_pending;
    S.join_pending = false;
    const bool ext_events = launch_events_allowed(st);
    hipEvent_t aux_done = c->oct_ev[si][kTailMaxOct];  // the aux stream's early stages (join_pending)
    if (join_pending && !S.desc_first) HIPCHK(hipStreamWaitEvent(st, aux_done, 0));
    if (!S.detected) CHK(launch_detection(c, si, 0, m, 0, p.n_oct, st));
    // (early: refinement and orientation were enqueued inside the pyramid)
    if (!S.early)
        CHK(launch_refine_stage(c, si, S.cand.p, cnt + L.cand(), B.bc, S.ext.p, cnt + L.ext(), B.be, st));
    if (S.staged) HIPCHK(hipEventRecord(S.ev[2], st));
    if (!S.early) CHK(launch_orient_stage(c, si, S.ext.p, cnt + L.ext(), B.be, B.bk, st));
    HIPCHK(hipGetLastError());
    if (S.staged) HIPCHK(hipEventRecord(S.ev[3], st));
    hipStream_t os = S.desc_first ? c->own2 : st;  // the ordering stage's stream
    hipStream_t ds = st;                            // the descriptor stage's stream
    if (S.desc_first) {
        // the ordering stage needs every keypoint: the lane stream's (tail
        // octaves) and, when the join is pending, the aux stream's; the
        // descriptors then run on the aux stream right after its orientation
        // (the lane stream's is long done by then), saving the cross-stream
        // hop in front of them (~15 us per one-frame call)
        HIPCHK(hipEventRecord(S.oriented, st));
        HIPCHK(hipStreamWaitEvent(os, S.oriented, 0));
        if (join_pending) {
            HIPCHK(hipStreamWaitEvent(os, aux_done, 0));
            ds = c->aux[si];
            HIPCHK(hipStreamWaitEvent(ds, S.oriented, 0));
        }
    }
    // emission order: radix sort of the keys (padding sorts last)
    const uint32_t* order = S.vals_b.p;  // emission order -> kp index
    const int img_bits = img_bits_for(m);
    const int end_bit = kKeyImgShift + img_bits;
    const uint64_t pad = (end_bit >= 64) ? ~0ull : ((1ull << end_bit) - 1);
    const bool onesweep = c->opts.onesweep == 1 || (c->opts.onesweep == 2 && B.bk >= kOnesweepMinKeys);
    size_t tmp = sort_pairs_u64(nullptr, 0, S.keys_a.p, S.keys_b.p, S.vals_a.p, S.vals_b.p, B.bk, end_bit, os, onesweep);
    const int rb = 32 + img_bits;
    const uint64_t rpad = (1ull << rb) - 1;
    if (limit >= 0)
        tmp = std::max(tmp, sort_pairs_u64(nullptr, 0, S.keys_a.p, S.keys_b.p, S.vals_a.p, S.fin.p, B.bk, rb, os, onesweep));
    if (!tmp) return fail(SIFT_MI_EHIP, "radix sort sizing failed");
    if (tmp > S.sort_tmp.cap) {
        HIPCHK(hipStreamSynchronize(st));
        if (os != st) HIPCHK(hipStreamSynchronize(os));
        CHK(S.sort_tmp.ensure(tmp));
    }
    launch_make_sort_keys(S.kp.p, n_kp, B.bk, pad, S.keys_a.p, S.vals_a.p, os);
    if (!sort_pairs_u64(S.sort_tmp.p, S.sort_tmp.cap, S.keys_a.p, S.keys_b.p, S.vals_a.p, S.vals_b.p, B.bk,
                        end_bit, os, onesweep))
        return fail(SIFT_MI_EHIP, "radix sort failed");
    launch_frame_starts(S.keys_b.p, n_kp, B.bk, starts, os);
    // features_limit (src/lib.rs:156-161): per-frame plan on the device
    // (desc_first: the plan's launch signals S.ordered, no marker after it)
    bool ordered_signalled = false;
    {
        LaunchDoneEvent done(S.desc_first && ext_events && limit < 0 ? S.ordered : nullptr);
        launch_limit_plan(starts, n_kp, B.bk, (int)m, limit, cnt + L.out_cnt(), S.seg_off.p, S.out_off.p,
                          S.use_resp.p, n_out, os);
        ordered_signalled = done.taken();
    }
    if (limit >= 0) {
        // stable sort: response-descending within each frame, emission order on ties
        launch_make_resp_keys(S.kp.p, order, n_kp, B.bk, 0, rpad, S.keys_a.p, S.vals_a.p, os);
        if (!sort_pairs_u64(S.sort_tmp.p, S.sort_tmp.cap, S.keys_a.p, S.keys_b.p, S.vals_a.p, S.fin.p, B.bk, rb,
                            os, onesweep))
            return fail(SIFT_MI_EHIP, "response sort failed");
        launch_select(order, S.fin.p, S.seg_off.p, S.out_off.p, S.use_resp.p, (int)m, n_out, B.bk, S.vals_a.p, os);
        order = S.vals_a.p;
    }
    HIPCHK(hipGetLastError());
    if (S.desc_first && !ordered_signalled) HIPCHK(hipEventRecord(S.ordered, os));
    if (S.staged) HIPCHK(hipEventRecord(S.ev[4], st));
    // descriptors into this slot's outputs, once its previous copy-out is done
    if (S.pending_copy) HIPCHK(hipStreamWaitEvent(ds, S.copied, 0));
    DescLaunch DL{};
    DL.kp = S.kp.p;
    DL.idx = S.desc_first ? nullptr : order;
    DL.n = S.desc_first ? n_kp : n_out;
    DL.bound = B.bk;
    DL.work = cnt + L.work();
    DL.key_base = (uint64_t)frame_base << kKeyImgShift;
    DL.oct = p.view(arena_of(c, si));
    DL.img_base = 0;
    DL.out_kp = S.desc_first ? nullptr : S.out_kp.p;
    DL.out_key = S.desc_first ? nullptr : S.out_key.p;
    DL.out_desc = S.desc_first ? S.desc_kp.p : S.out_desc.p;
    DL.exact = c->exact_descriptors;
    DL.samples = c->count_samples ? c->samples.p + 8 : nullptr;
    launch_describe(DL, ds);
    bool counts_copied = false;  // by k_gather_out, which then signals ev[6] itself
    if (S.desc_first) {
        HIPCHK(hipStreamWaitEvent(ds, S.ordered, 0));
        const bool in_gather = ext_events && !S.staged;
        LaunchDoneEvent done(in_gather ? S.ev[6] : nullptr);
        launch_gather_out(S.kp.p, order, n_out, B.bk, S.desc_kp.p, S.out_desc.p, S.out_kp.p, S.out_key.p,
                          DL.key_base, in_gather ? cnt : nullptr, in_gather ? S.h_counts.p : nullptr,
                          (int)L.host_words(), ds);
        counts_copied = done.taken();
    }
    HIPCHK(hipGetLastError());
    if (S.staged) HIPCHK(hipEventRecord(S.ev[5], st));
    if (!counts_copied) {
        HIPCHK(hipMemcpyAsync(S.h_counts.p, cnt, L.host_words() * sizeof(uint32_t), hipMemcpyDeviceToHost, ds));
        HIPCHK(hipEventRecord(S.ev[6], ds));
    }
    // the lane stream's next work follows this chunk (and a capture rejoins)
    if (ds != st) HIPCHK(hipStreamWaitEvent(st, S.ev[6], 0));
    return 0;
}

void accumulate_times(sift_mi_ctx* c, Slot& S) {
    float ms;
    // (a graph replay records only the chunk's ends)
    if (S.graph_run && hipEventElapsedTime(&ms, S.ev[0], S.ev[6]) == hipSuccess) c->stats.total_ms += ms;
    if (S.graph_run || !S.staged) return;
    if (hipEventElapsedTime(&ms, S.ev[0], S.ev[1]) == hipSuccess) c->stats.pyramid_ms += ms;
    if (hipEventElapsedTime(&ms, S.ev[1], S.ev[2]) == hipSuccess) c->stats.detect_ms += ms;
    if (hipEventElapsedTime(&ms, S.ev[2], S.ev[3]) == hipSuccess) c->stats.orient_ms += ms;
    if (hipEventElapsedTime(&ms, S.ev[3], S.ev[4]) == hipSuccess) c->stats.order_ms += ms;
    if (hipEventElapsedTime(&ms, S.ev[4], S.ev[5]) == hipSuccess) c->stats.descriptor_ms += ms;
    if (hipEventElapsedTime(&ms, S.ev[0], S.ev[6]) == hipSuccess) c->stats.total_ms += ms;
}

// Enqueue pyramid (optional) + keypoint stages of one chunk on slot si.
int enqueue_chunk(sift_mi_ctx* c, int si, const uint8_t* d_frames, size_t frame_pitch, size_t stride, uint32_t m,
                  int64_t limit, uint32_t frame_base, bool pyramid) {
    Slot& S = c->slot[si];
    const Bounds B = chunk_bounds(c, m);
    CHK(ensure_lane(c, arena_of(c, si)));
    CHK(reserve_chunk(c, si, B, c->plan.chunk, m));
    hipStream_t st = lane_stream(c, si);
    S.staged = c->lanes == 1;
    if (S.staged) HIPCHK(hipEventRecord(S.ev[0], st));
    CHK(prepare_chunk(c, si, m, frame_base, B, pyramid));
    // stage overlap (two-lane mode; the one-lane mode times the stages apart):
    // detection starts inside the pyramid (run_pyramid), so ev[1]..ev[2] is
    // then only the refinement
    const bool fused = pyramid && c->lanes == 2;
    if (pyramid) CHK(run_pyramid(c, si, d_frames, frame_pitch, stride, m, false, fused ? si : -1, si));
    flush_chunk_init(c, si);  // (run_pyramid launched it after the seed)
    if (S.staged) HIPCHK(hipEventRecord(S.ev[1], st));
    return enqueue_keypoints(c, si, m, limit, frame_base, B);
}

// Slot S's n_out results behind `base` rows of (kp, desc, key), on the copy
// stream once the chunk is done.
int copy_results(sift_mi_ctx* c, Slot& S, OutKp* kp, uint8_t* desc, uint64_t* key, size_t base, uint32_t n_out,
                 hipMemcpyKind kind) {
    HIPCHK(hipStreamWaitEvent(c->cstream, S.ev[6], 0));
    HIPCHK(hipMemcpyAsync(kp + base, S.out_kp.p, n_out * sizeof(OutKp), kind, c->cstream));
    HIPCHK(hipMemcpyAsync(desc + base * kDescSize, S.out_desc.p, (size_t)n_out * kDescSize, kind, c->cstream));
    HIPCHK(hipMemcpyAsync(key + base, S.out_key.p, n_out * sizeof(uint64_t), kind, c->cstream));
    HIPCHK(hipEventRecord(S.copied, c->cstream));
    S.pending_copy = true;
    return 0;
}

// Wait for slot si's chunk; on success append its per-frame offsets and start
// the copy of its results to the host.  Returns 1 when a stage count exceeded
// its bound (the caller re-runs the chunk; the high-water marks now cover it).
int finalize_chunk(sift_mi_ctx* c, int si, size_t* offsets, bool only_chunk = false) {
    Slot& S = c->slot[si];
    HIPCHK(host_wait_event(S.ev[6]));
    const uint32_t* h = S.h_counts.p;
    const uint32_t m = S.m;
    const CounterLayout L = S.layout();
    const double fm = (double)m;
    // the tail octaves' region (Slot::early): its counts follow the frame plan
    const uint32_t hb0 = S.early ? h[L.tail_cand()] : 0, hb1 = S.early ? h[L.tail_ext()] : 0;
    // the main region's extrema (a two-ended append keeps its back count in the tail words)
    const uint32_t h1 = h[L.ext()] + (S.early ? h[L.ext_back()] : 0);
    c->pf_cand = std::max(c->pf_cand, (h[L.cand()] + hb0) / fm);
    c->pf_ext = std::max(c->pf_ext, (h1 + hb1) / fm);
    c->pf_kp = std::max(c->pf_kp, h[L.kp()] / fm);
    c->pf_cand_b = std::max(c->pf_cand_b, std::max(hb0, hb1) / fm);
    if (h[L.cand()] > S.bc || h1 > S.be || h[L.kp()] > S.bk || hb0 > S.bcb || hb1 > S.bcb) {
        c->stats.stage_reruns++;
        return 1;
    }
    const uint32_t n_out = h[L.out()];
    accumulate_times(c, S);
    const size_t base = c->n_rows, need = base + n_out;
    const bool to_device = c->call_dest == ResultWhere::device;
    if (offsets) {
        size_t acc = base;
        for (uint32_t f = 0; f < m; f++) {
            offsets[S.frame_base + f] = acc;
            acc += h[L.out_cnt() + f];
        }
    }
    c->res_slot = -1;
    if (to_device && only_chunk) {
        // the call's only chunk: its outputs ARE the batch's device results
        // (valid until the next call, sift_mi_device_results) -- no copy
        c->res_slot = si;
    } else if (to_device) {
        // whole-batch device arena: device-to-device copies on the copy stream
        if (n_out && (need > c->r_kp.cap || need * kDescSize > c->r_desc.cap || need > c->r_key.cap)) {
            HIPCHK(hipStreamSynchronize(c->cstream));
            CHK(grow_keep(c->r_kp, need, base, c->cstream));
            CHK(grow_keep(c->r_desc, need * kDescSize, base * kDescSize, c->cstream));
            CHK(grow_keep(c->r_key, need, base, c->cstream));
        }
        if (n_out) CHK(copy_results(c, S, c->r_kp.p, c->r_desc.p, c->r_key.p, base, n_out, hipMemcpyDeviceToDevice));
    } else {
        if (need > c->h_kp.cap || need * kDescSize > c->h_desc.cap || need > c->h_key.cap) {
            HIPCHK(hipStreamSynchronize(c->cstream));  // copies in flight into the old buffers
            CHK(c->h_kp.ensure(need, true));
            CHK(c->h_desc.ensure(need * kDescSize, true));
            CHK(c->h_key.ensure(need, true));
        }
        if (n_out) CHK(copy_results(c, S, c->h_kp.p, c->h_desc.p, c->h_key.p, base, n_out, hipMemcpyDeviceToHost));
    }
    c->n_rows = need;
    c->stats.extrema += h1 + hb1;
    c->stats.keypoints += n_out;
    c->stats.frames += m;
    return 0;
}

// A single-chunk call replayed as a HIP graph (PathOpts::graph): the first
// call with a given key runs normally (it also sizes every buffer), the
// second identical one is captured (relaxed stream capture of enqueue_chunk:
// the fork / join with the aux stream becomes graph edges) and launched, later
// ones only launch the graph.  Any (re)allocation changes the key (its
// buffers are baked into the graph).  Returns 1 when the chunk was enqueued
// here, 0 when the caller must enqueue it.
int enqueue_single_graph(sift_mi_ctx* c, const uint8_t* d_frames, size_t frame_pitch, size_t stride, uint32_t m,
                         int64_t limit) {
    Slot& S = c->slot[0];
    if (!c->opts.graph || c->band_n > 1 || c->lanes != 2 || S.pending_copy) return 0;
    const Bounds B = chunk_bounds(c, m);
    CHK(ensure_lane(c, arena_of(c, 0)));
    CHK(reserve_chunk(c, 0, B, c->plan.chunk, m));
    hipStream_t st = lane_stream(c, 0);
    sift_mi_ctx::GraphKey k;
    std::memset(&k, 0, sizeof k);
    k.opts = c->opts;
    k.frames = d_frames;
    k.frame_pitch = frame_pitch;
    k.stride = stride;
    k.m = m;
    k.w = c->plan.w;
    k.h = c->plan.h;
    k.bc = B.bc;
    k.be = B.be;
    k.bk = B.bk;
    k.bcb = S.bcb;
    k.limit = limit;
    k.gen = g_alloc_gen.load();
    k.keep = c->call_dest == ResultWhere::device;
    k.exact = c->exact_descriptors;
    k.samples = c->count_samples;
    k.lanes = c->lanes;
    k.prof = c->plan.profile;
    k.maxo = c->plan.max_oct;
    k.st = st;
    if (!(c->gkey_ok && c->gkey == k)) {
        if (!(c->gseen_ok && c->gseen == k)) {  // first sighting: a normal run
            c->gseen = k;
            c->gseen_ok = true;
            return 0;
        }
        c->gkey_ok = false;
        if (c->gexec) (void)hipGraphExecDestroy(c->gexec);
        if (c->graph) (void)hipGraphDestroy(c->graph);
        c->gexec = nullptr;
        c->graph = nullptr;
        const sift_mi_stats stats0 = c->stats;
        HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
        const int rc = enqueue_chunk(c, 0, d_frames, frame_pitch, stride, m, limit, 0, true);
        hipGraph_t g = nullptr;
        const hipError_t e = hipStreamEndCapture(st, &g);
        if (rc || e != hipSuccess || !g) {
            if (g) (void)hipGraphDestroy(g);
            c->gseen_ok = false;
            return rc ? rc : fail(SIFT_MI_EHIP, std::string("graph capture failed: ") + hipGetErrorString(e));
        }
        if (g_alloc_gen.load() != k.gen) {
            // something was (re)allocated during the capture.  The counter is
            // process-wide, so this is another context on another thread, or
            // this context itself (a buffer grown inside enqueue_chunk); in
            // neither case an error.  The capture ran nothing, so drop the
            // graph and let the caller enqueue the chunk plainly: that run
            // uses the buffers as they now are.  The next identical call
            // starts over as a first sighting.  (A neighbour that allocates
            // steadily keeps moving the key, so no graph is captured beside
            // it: slower, not wrong.)
            (void)hipGraphDestroy(g);
            c->gseen_ok = false;
            c->stats = stats0;  // (the plain run counts its launches itself)
            return 0;
        }
        if (hipGraphInstantiate(&c->gexec, g, nullptr, nullptr, 0) != hipSuccess) {
            (void)hipGraphDestroy(g);
            c->gexec = nullptr;
            c->gseen_ok = false;
            return fail(SIFT_MI_EHIP, "hipGraphInstantiate failed");
        }
        c->graph = g;
        c->gkey = k;
        c->gkey_ok = true;
        c->g_early = S.early;
        c->g_fused = S.fused_mask;
    }
    // the replay runs what the captured chunk ran
    set_chunk_state(S, m, 0, B);
    S.detected = true;
    S.graph_run = true;
    S.early = c->g_early;
    S.fused_mask = c->g_fused;
    HIPCHK(hipEventRecord(S.ev[0], st));
    HIPCHK(hipGraphLaunch(c->gexec, st));
    HIPCHK(hipEventRecord(S.ev[6], st));
    return 1;
}

}  // namespace

int ensure_plan(sift_mi_ctx* c, uint32_t w, uint32_t h, uint32_t chunk) {
    Plan& p = c->plan;
    const bool same = p.w == w && p.h == h && p.profile == (int)c->profile && p.max_oct == c->max_octaves;
    if (same && p.chunk >= chunk && p.arena[0].p) return 0;
    // the arenas are re-sized or re-planned: the caller is a producing call
    // (ProducingScope), which no earlier pyramid or batch read-back survives
    if (!same) {
        p = Plan{};  // nothing of the old plan is kept
        // per-frame stage high-water marks belong to a frame size
        c->pf_cand = c->pf_ext = c->pf_kp = 0;
        c->pf_cand_b = 0;
    }
    p.profile = (int)c->profile;
    const bool ip = c->profile == SIFT_MI_PROFILE_IMAGEPROC;
    p.w = w;
    p.h = h;
    p.chunk = chunk;
    int n_oct = n_octaves_for(w, h);
    // labelled extension (sift_mi_set_max_octaves): fewer octaves than the
    // crate's formula (src/lib.rs:133-134); the kept octaves are unchanged
    if (c->max_octaves > 0) n_oct = std::min(n_oct, c->max_octaves);
    p.max_oct = c->max_octaves;
    if (!octave_geometry(w, h, n_oct, chunk, p)) return fail(SIFT_MI_EINVAL, "image too small for the octave count");
    // nearest 1/2 must be source pixel (2x, 2y) (OpenCV INTER_NEAREST) or
    // (2x + 1, 2y + 1) (image Nearest) for the fused epilogue
    for (int o = 0; o + 1 < p.n_oct; o++)
        for (const int src : {p.ow[o], p.oh[o]}) {
            const int bad = nearest_half_check(src, ip);
            if (bad == 1) return fail(SIFT_MI_EUNSUPPORTED, "nearest 1/2 with more than one tap");
            if (bad) return fail(SIFT_MI_EUNSUPPORTED, "nearest 1/2 offset is not 2x (+1)");
        }
    // algorithmic bytes: the u8 frame read once and every
    // image of PrecomputedImages (G_0..G_5, D_0..D_4: 44 B per octave pixel)
    // written once -- the fixed yardstick for every path.  The batch path
    // itself writes only G_0..G_5 and forms D where detection reads it, so
    // its pyramid kernels move ~44 B per octave pixel counting their reads
    // (DESIGN.md 3.1).
    p.algo_bytes_per_frame = (uint64_t)w * h + 44ull * p.sum_px;
    for (int l = 0; l < 2; l++) {  // a larger chunk re-sizes both lanes
        p.arena[l].release();
        p.d_gauss[l].release();
    }
    hipStream_t st = c->stream;
    if (ip)
        CHK(p.seed_iptab.upload((int)w, (int)h, 2 * (int)w, 2 * (int)h, 1.0f, kIpTaps, st));
    else
        CHK(p.seed_tab.upload((int)w, (int)h, 2 * (int)w, 2 * (int)h, st));
    if (ip && (p.seed_iptab.xtaps > kIpTaps || p.seed_iptab.ytaps > kIpTaps))
        return fail(SIFT_MI_EUNSUPPORTED, "2x Triangle upsample with more than 3 taps");
    std::vector<size_t> gs(p.n_oct);
    for (int o = 0; o < p.n_oct; o++) gs[o] = p.gstride(o);
    CHK(upload(p.d_gstride, gs.data(), p.n_oct, st));
    CHK(upload(p.d_ow, p.ow.data(), p.n_oct, st));
    CHK(upload(p.d_oh, p.oh.data(), p.n_oct, st));
    CHK(upload(p.d_opitch, p.opitch.data(), p.n_oct, st));
    HIPCHK(hipStreamSynchronize(st));
    // P::gaussian_blur(img, sigma: f64); ImageprocProcessing passes sigma as f32
    p.seed_r = ip ? ip_blur_taps((float)seed_sigma(), &p.seed_taps) : cv_blur_taps(seed_sigma(), &p.seed_taps);
    double sig[kImagesPerOctave];
    octave_sigmas(sig);
    for (int s = 1; s < kImagesPerOctave; s++)
        p.oct_r[s] = ip ? ip_blur_taps((float)sig[s], &p.oct_taps[s]) : cv_blur_taps(sig[s], &p.oct_taps[s]);
    return ensure_lane(c, 0);
}

int run_pyramid(sift_mi_ctx* c, int lane, const uint8_t* d_frames, size_t frame_pitch, size_t row_stride,
                uint32_t n, bool full, int detect_slot, int cand_slot) {
    Plan& p = c->plan;
    if (full && n != 1) return fail(SIFT_MI_EINVAL, "the DoG planes are materialised for one frame");
    hipStream_t st = lane_stream(c, lane);
    lane = arena_of(c, lane);
    PyramidRun R{c, p, c->opts, lane, c->aux[lane], lane == 0 ? c->aux2 : nullptr, d_frames, frame_pitch,
                 row_stride, full, detect_slot, cand_slot};
    c->band_restricted = c->band_n > 1 && !full && !c->band_whole && p.profile == (int)SIFT_MI_PROFILE_OPENCV;
    if (c->band_restricted) {
        R.rows = band_rows(p.oh.data(), p.n_oct, p.oct_r, c->band_r, c->band_n);
        R.seed_y0 = R.row_lo(0, 0);
        R.seed_y1 = std::max(R.row_hi(0, 0), R.seed_y0 + 1);
    }
    R.o_tail = p.n_oct;
    if (c->opts.tail && p.n_oct <= kTailMaxOct)
        R.o_tail = tail_octave_start(p.ow.data(), p.oh.data(), p.n_oct, p.oct_r);
    R.ext_events = launch_events_allowed(st);
    uint64_t bytes = p.algo_bytes_per_frame;  // per frame, SURVEY.md 8(d)
    if (c->band_restricted) {
        // the same yardstick over the rows this band computes: 4 B per pixel
        // of each of its 6 Gaussian rows and 5 DoG rows, plus the input rows
        // the seed reads; the tail launch computes its octaves whole
        double b = (double)p.w * std::min<int>((int)p.h, (R.seed_y1 - R.seed_y0 + 1) / 2 + 2);
        for (int o = 0; o < p.n_oct; o++) {
            double rows = 0;
            for (int s = 0; s < kImagesPerOctave; s++) {
                const int r = o >= R.o_tail ? p.oh[o] : std::max(0, R.row_hi(o, s) - R.row_lo(o, s));
                rows += (s < kDogPerOctave ? 2.0 : 1.0) * r;
            }
            b += 4.0 * p.ow[o] * rows;
        }
        bytes = (uint64_t)b;
    }
    // octave overlap only while the other lane is idle: with two chunks in
    // flight the other lane's kernels already fill the chip, and the extra
    // stream costs ~2% of batch throughput (30.4 vs 29.8 M keypoints/s,
    // 128 1080p frames, three A/B pairs)
    CHK(R.part(0, n, st, !c->lanes_busy && p.n_oct <= kTailMaxOct));
    HIPCHK(hipGetLastError());
    c->stats.pyramid_launches += R.launches;
    // pyramid_bytes is SURVEY.md 8(d)'s yardstick alone (W*H + 44*sum P_o per
    // frame).  The octaves whose extremum scan ran inside the stage
    // (k_blur_detect) are reported apart: what the reference's scan reads for
    // them, the five DoG planes once (20 B per octave pixel), so a caller can
    // state the fused stage's figure without mixing the two yardsticks.
    uint64_t scan = 0;
    if (cand_slot >= 0)
        for (int o = 0; o < p.n_oct && o < 32; o++)
            if ((c->slot[cand_slot].fused_mask >> o) & 1) scan += 20ull * p.px[o];
    c->stats.pyramid_bytes += bytes * n;
    c->stats.pyramid_scan_bytes += scan * n;
    return 0;
}

int run_chunk_sync(sift_mi_ctx* c, const uint8_t* d_frames, size_t frame_pitch, size_t stride, uint32_t m,
                   int64_t limit, bool pyramid, size_t* offsets) {
    CHK(check_band_limit(c, limit));  // (the caller has checked it before touching anything)
    c->n_rows = 0;
    for (int attempt = 0; attempt < 4; attempt++) {
        CHK(enqueue_chunk(c, 0, d_frames, frame_pitch, stride, m, limit, 0, pyramid));
        const int rc = finalize_chunk(c, 0, offsets);
        if (rc < 0) return rc;
        if (rc == 0) {
            if (offsets) offsets[m] = c->n_rows;
            HIPCHK(hipStreamSynchronize(c->cstream));
            return 0;
        }
    }
    return fail(SIFT_MI_ENOMEM, "stage count kept exceeding its buffer bound");
}

// Chunks alternate between two lanes (slot, stream, pyramid arena and stage
// buffers each), so chunk k+1's kernels run beside chunk k's -- the small
// octaves, sorts and kernel tails of one chunk leave CUs idle that the other
// fills -- and chunk k+2 is enqueued as soon as chunk k has been finalised.
// Results travel on the copy stream.
int check_band_limit(const sift_mi_ctx* c, int64_t limit) {
    if (c->band_n > 1 && limit >= 0)
        return fail(SIFT_MI_EINVAL, "features_limit ranks a whole frame's keypoints: apply it after merging row bands");
    return 0;
}

int check_extract_args(const sift_mi_ctx* c, uint32_t n, uint32_t w, uint32_t h, size_t stride, int64_t limit) {
    CHK(check_frame_args(w, h, stride));
    if (n > (1u << (64 - kKeyImgShift))) return fail(SIFT_MI_EINVAL, "more than 2^22 frames in one call (key field)");
    return check_band_limit(c, limit);
}

namespace {
// The call proper, after the argument checks; *one_chunk: it ran as one chunk
// whose planes are whole (the batch read-back).  Calls itself once to redo a
// row band on the whole-frame pyramid.
int extract_run(sift_mi_ctx* c, const uint8_t* d_frames, size_t frame_pitch, uint32_t n, uint32_t w, uint32_t h,
                size_t stride, int64_t limit, size_t* offsets, bool* one_chunk) {
    const sift_mi_stats stats0 = c->stats;  // restored if a banded pass is redone on the whole pyramid
    unsigned long long samples0[16] = {};   // and the device sample counters with it
    if (c->band_n > 1 && c->count_samples && c->samples.p) {
        CHK(sync_lanes(c));
        HIPCHK(hipMemcpy(samples0, c->samples.p, sizeof samples0, hipMemcpyDeviceToHost));
    }
    double avail = 0;  // device memory this context could hold: free + its own arenas
    if (!c->chunk_override && n > 1) {  // (one frame is one chunk: no query on the latency path)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            avail = (double)free_b + 4.0 * ((double)c->plan.arena[0].cap + (double)c->plan.arena[1].cap);
    }
    const uint32_t chunk = std::min(kMaxChunk, c->chunk_override ? std::min(c->chunk_override, n)
                                                                 : auto_chunk(w, h, n, c->opts.chunk_mode, avail));
    CHK(ensure_plan(c, w, h, chunk));
    c->n_rows = 0;
    *one_chunk = false;
    if (c->band_n > 1) {
        CHK(c->band_flag.ensure(1));
        HIPCHK(hipMemsetAsync(c->band_flag.p, 0, sizeof(uint32_t), c->stream));
    }
    const uint32_t n_chunks = (n + chunk - 1) / chunk;
    auto frames_of = [&](uint32_t k) { return std::min(chunk, n - k * chunk); };
    auto enqueue = [&](uint32_t k) {
        return enqueue_chunk(c, (int)(k & 1), d_frames + (size_t)k * chunk * frame_pitch, frame_pitch, stride,
                             frames_of(k), limit, k * chunk, true);
    };
    // lane 1 starts after the caller's stream (frames produced there); the
    // caller's stream resumes after lane 1's last chunk
    const bool two = n_chunks > 1 && c->lanes == 2;
    c->lanes_busy = two;
    struct Reset {
        sift_mi_ctx* c;
        ~Reset() { c->lanes_busy = false; }
    } reset_busy{c};
    if (two) {
        HIPCHK(hipEventRecord(c->fork, c->stream));
        HIPCHK(hipStreamWaitEvent(c->own2, c->fork, 0));
    }
    if (n_chunks == 1) {
        const int g = enqueue_single_graph(c, d_frames, frame_pitch, stride, n, limit);
        if (g < 0) return g;
        if (g == 0) CHK(enqueue(0));
    } else {
        CHK(enqueue(0));
        CHK(enqueue(1));
    }
    for (uint32_t k = 0; k < n_chunks; k++) {
        int rc = finalize_chunk(c, (int)(k & 1), offsets, n_chunks == 1);
        if (rc < 0) return rc;
        for (int attempt = 0; rc == 1; attempt++) {
            // a stage overflowed its bound: drain both lanes (the other lane's
            // chunk is unaffected), then re-run k on its lane
            if (attempt == 3) return fail(SIFT_MI_ENOMEM, "stage count kept exceeding its buffer bound");
            CHK(sync_lanes(c));
            CHK(enqueue(k));
            rc = finalize_chunk(c, (int)(k & 1), offsets, n_chunks == 1);
            if (rc < 0) return rc;
        }
        if (k + 2 < n_chunks) CHK(enqueue(k + 2));
    }
    if (two) {
        HIPCHK(hipEventRecord(c->fork, c->own2));
        HIPCHK(hipStreamWaitEvent(c->stream, c->fork, 0));
    }
    // every copy of the call done (a device-resident one-chunk call copied
    // nothing: no synchronisation, whose marker round trip costs a few us)
    if (c->slot[0].pending_copy || c->slot[1].pending_copy) HIPCHK(hipStreamSynchronize(c->cstream));
    for (auto& S2 : c->slot) S2.pending_copy = false;
    if (offsets) offsets[n] = c->n_rows;
    if (n_chunks == 1 && !c->band_restricted) {
        *one_chunk = true;
        c->batch_arena = arena_of(c, 0);
        c->batch_frames = n;
    }
    if (c->band_restricted) {
        // a refinement drifted past the computed rows: redo the band on the
        // whole-frame pyramid (exact; the rare case)
        c->band_restricted = false;
        uint32_t flag = 0;
        HIPCHK(hipMemcpy(&flag, c->band_flag.p, sizeof(flag), hipMemcpyDeviceToHost));
        if (flag) {
            // the first pass's work is discarded: report the re-run alone
            const uint64_t reruns = c->stats.band_reruns + 1, stage_reruns = c->stats.stage_reruns;
            c->stats = stats0;
            c->stats.band_reruns = reruns;
            c->stats.stage_reruns = stage_reruns;
            if (c->count_samples && c->samples.p)
                HIPCHK(hipMemcpy(c->samples.p, samples0, sizeof samples0, hipMemcpyHostToDevice));
            c->band_whole = true;
            const int rc = extract_run(c, d_frames, frame_pitch, n, w, h, stride, limit, offsets, one_chunk);
            c->band_whole = false;
            return rc;
        }
    }
    return 0;
}
}  // namespace

int extract_device(sift_mi_ctx* c, ProducingCall call, const uint8_t* d_frames, size_t frame_pitch, uint32_t n,
                   uint32_t w, uint32_t h, size_t stride, int64_t limit, size_t* offsets) {
    CHK(check_extract_args(c, n, w, h, stride, limit));  // refused for its arguments: nothing changes
    // from here on the plan, the arenas and the result buffers are rewritten
    ProducingScope<> scope(c->rs);
    c->call_dest = c->rs.destination(call);
    bool one_chunk = false;
    CHK(extract_run(c, d_frames, frame_pitch, n, w, h, stride, limit, offsets, &one_chunk));
    scope.done(call, c->call_dest, c->n_rows, one_chunk);
    return 0;
}

}  // namespace siftmi
