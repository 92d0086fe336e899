// Brute-force descriptor matching on the MFMA units (SURVEY.md 8(f) row 3:
// the step after the path).
//
// Reference: examples/sift-match.rs:30-35 matches two SiftResults with
// cv::BFMatcher(NORM_L2, crossCheck = true).match(query, train):
//   * distance = sqrt((float) sum (q_k - t_k)^2), the integer sum exact
//     (batchDistL2_8u32f);
//   * each query's nearest train row, lowest index on ties (strict <);
//   * cross check keeps query i only if its nearest train row's nearest query
//     is i (cv::batchDistance crosscheck); matches come out in query order.
//
// Dot products run as bf16 MFMA (mfma_f32_32x32x16_bf16): u8 values are exact
// in bf16 and every partial sum (< 128 * 255^2 < 2^24) is an exact f32
// integer, so d^2 = |q|^2 + |t|^2 - 2 q.t is the exact integer.  A 256-thread
// workgroup owns a 128 x 128 (query x train) tile, each wave 64 x 64 (2 x 2
// MFMA tiles, 8 k-steps); the tile's row / column minima are folded into
// global per-query and per-train (d^2 << 32 | index) keys with 64-bit
// atomicMin, which also gives the lowest-index tie break.
#include "match_common.h"

namespace siftmi {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ short u8_to_bf16(uint32_t v) {
    return (short)(__float_as_uint((float)v) >> 16);  // exact for 0..255
}

// 8 consecutive u8 of one descriptor row -> bf16 MFMA fragment
__device__ __forceinline__ bf16x8 load_frag(const uint8_t* __restrict__ base, int row, int n, int k0) {
    bf16x8 f;
    if (row < n) {
        const uint2 w = *reinterpret_cast<const uint2*>(base + (size_t)row * kDescSize + k0);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            f[j] = u8_to_bf16((w.x >> (8 * j)) & 0xff);
            f[4 + j] = u8_to_bf16((w.y >> (8 * j)) & 0xff);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) f[j] = 0;
    }
    return f;
}

__global__ __launch_bounds__(256) void k_match_norms(const uint8_t* __restrict__ d, int n, float* __restrict__ nrm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint4* p = reinterpret_cast<const uint4*>(d + (size_t)i * kDescSize);
    uint32_t s = 0;
#pragma unroll
    for (int c = 0; c < kDescSize / 16; c++) {
        const uint4 w = p[c];
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t b = (ws[q] >> (8 * j)) & 0xff;
                s += b * b;
            }
    }
    nrm[i] = (float)s;  // < 2^24: exact
}

__device__ __forceinline__ uint64_t min_u64(uint64_t a, uint64_t b) { return a < b ? a : b; }

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(256) void k_match_tiles(const uint8_t* __restrict__ q, int nq,
                                                     const uint8_t* __restrict__ t, int nt,
                                                     const float* __restrict__ qn, const float* __restrict__ tn,
                                                     unsigned long long* __restrict__ row_best,
                                                     unsigned long long* __restrict__ col_best) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * 128 + (wave >> 1) * 64;  // this wave's 64 query rows
    const int t0 = blockIdx.y * 128 + (wave & 1) * 64;   // and 64 train rows
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[a][b][e] = 0.0f;
#pragma unroll
    for (int s = 0; s < kDescSize / 16; s++) {
        const int k0 = 16 * s + 8 * h;
        bf16x8 fa[2], fb[2];
#pragma unroll
        for (int a = 0; a < 2; a++) fa[a] = load_frag(q, q0 + 32 * a + r, nq, k0);
#pragma unroll
        for (int b = 0; b < 2; b++) fb[b] = load_frag(t, t0 + 32 * b + r, nt, k0);
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++)
                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
    // C/D: column (train) = lane & 31, row (query) = (e & 3) + 8 * (e >> 2) + 4 * h
    const uint64_t INF = ~0ull;
    float tnorm[2];
    int tc[2];
#pragma unroll
    for (int b = 0; b < 2; b++) {
        tc[b] = t0 + 32 * b + r;
        tnorm[b] = tc[b] < nt ? tn[tc[b]] : 0.0f;
    }
    uint64_t colmin[2] = {INF, INF};
#pragma unroll
    for (int a = 0; a < 2; a++) {
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int qr = q0 + 32 * a + (e & 3) + 8 * (e >> 2) + 4 * h;
            const float qnv = qr < nq ? qn[qr] : 0.0f;
            uint64_t rowkey = INF;
#pragma unroll
            for (int b = 0; b < 2; b++) {
                const float d2 = qnv + tnorm[b] - 2.0f * acc[a][b][e];  // exact integer
                const bool valid = qr < nq && tc[b] < nt;
                const uint32_t di = (uint32_t)d2;
                const uint64_t kr = valid ? ((uint64_t)di << 32) | (uint32_t)tc[b] : INF;
                const uint64_t kc = valid ? ((uint64_t)di << 32) | (uint32_t)qr : INF;
                rowkey = min_u64(rowkey, kr);
                colmin[b] = min_u64(colmin[b], kc);
            }
            // row minimum over the 32 train columns of this lane half
#pragma unroll
            for (int m = 16; m >= 1; m >>= 1) rowkey = min_u64(rowkey, shfl_xor_u64(rowkey, m));
            if (r == 0 && rowkey != INF) atomicMin(&row_best[qr], (unsigned long long)rowkey);
        }
    }
    // column minimum over both lane halves
#pragma unroll
    for (int b = 0; b < 2; b++) {
        const uint64_t k = min_u64(colmin[b], shfl_xor_u64(colmin[b], 32));
        if (h == 0 && k != INF) atomicMin(&col_best[tc[b]], (unsigned long long)k);
    }
}

__global__ __launch_bounds__(256) void k_match_final(const unsigned long long* __restrict__ row_best,
                                                     const unsigned long long* __restrict__ col_best, int nq,
                                                     int cross_check, int* __restrict__ train_idx,
                                                     float* __restrict__ dist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    const uint64_t rb = row_best[i];
    int tix = -1;
    float d = 0.0f;
    if (rb != ~0ull) {
        const int tt = (int)(uint32_t)rb;
        if (!cross_check || (int)(uint32_t)col_best[tt] == i) {
            tix = tt;
            d = sqrtf((float)(uint32_t)(rb >> 32));  // batchDistL2_8u32f: sqrt((float) int)
        }
    }
    train_idx[i] = tix;
    dist[i] = d;
}

void launch_match(const uint8_t* q, int nq, const uint8_t* t, int nt, int cross_check, float* qn, float* tn,
                  unsigned long long* row_best, unsigned long long* col_best, int* train_idx, float* dist,
                  hipStream_t st) {
    if (nq <= 0) return;
    (void)hipMemsetAsync(row_best, 0xff, (size_t)nq * 8, st);
    if (nt > 0) (void)hipMemsetAsync(col_best, 0xff, (size_t)nt * 8, st);
    hipLaunchKernelGGL(k_match_norms, dim3((nq + 255) / 256), dim3(256), 0, st, q, nq, qn);
    if (nt > 0) {
        hipLaunchKernelGGL(k_match_norms, dim3((nt + 255) / 256), dim3(256), 0, st, t, nt, tn);
        hipLaunchKernelGGL(k_match_tiles, dim3((nq + 127) / 128, (nt + 127) / 128), dim3(256), 0, st, q, nq, t, nt, qn,
                           tn, row_best, col_best);
    }
    hipLaunchKernelGGL(k_match_final, dim3((nq + 255) / 256), dim3(256), 0, st, row_best, col_best, nq, cross_check,
                       train_idx, dist);
}

// ---- segmented 2-NN matching: many (query segment, train segment) pairs of
// one descriptor arena in one launch sequence ----------------
//
// LABELLED EXTENSION: cv::BFMatcher(NORM_L2).knnMatch(query, train, 2) and the
// Lowe ratio test on it.  d^2 is the exact integer, as in k_match_tiles, here
// through the i8 MFMA (mfma_i32_32x32x32_i8, twice the bf16 form's rate and no
// u8 -> bf16 conversion in front of it): with x' = x - 128 (one xor per four
// bytes) q.t = q'.t' + 128 (sum q + sum t) - 2^21, so
//     d^2 = m_q + m_t + 2^22 - 2 q'.t',   m_x = |x|^2 - 256 sum x,
// every term an i32 (|q'.t'| <= 2^21).  A workgroup owns a 128 x 128 tile of
// ONE pair (each wave 64 x 64: 2 x 2 MFMA tiles, 4 k-steps), found by bisecting the
// pairs' tile prefix (MatchPair::tile0) with its 1-D block index.  Rows and
// columns are valid against the pair's segment lengths: the rows past a
// segment are the next frame's, readable and wrong.
//
// Top 2 per query: the keys (d^2 << 32 | train index) of one query are
// distinct.  A wave reduces its 64 columns to the row's two smallest keys
// (lo < hi) and folds them into two global slots:
//     old = atomicMin(&best[q], lo); atomicMin(&second[q], max(old, lo));
//     atomicMin(&second[q], hi);
// The true minimum g never loses at `best`, so it is never the max of such an
// exchange and never reaches `second`.  The true second minimum s reaches it:
// as a wave's hi (then g is that wave's lo), as the loser on arrival (g
// already in `best`), or when g later displaces it from `best`.  Everything
// else that reaches `second` is larger, so the final state is (g, s) for
// every arrival order and every tiling.

// The in-wave 32-bit keys, merge2 / fold_rows, pair_of and load_frag_i8 are in
// match_common.h (the guided tile kernel of match_guided.hip uses them too).

// Per row of the segments some pair uses, m = |row|^2 - 256 * sum(row) (the
// row's part of d^2 in the biased i8 form, below); blocks[b] = (first arena
// row, rows <= 256)
__global__ __launch_bounds__(256) void k_match_seg_norms(const uint8_t* __restrict__ d,
                                                         const uint2* __restrict__ blocks,
                                                         int* __restrict__ nrm) {
    const uint2 blk = blocks[blockIdx.x];
    if (threadIdx.x >= blk.y) return;
    const size_t i = (size_t)blk.x + threadIdx.x;
    const uint4* p = reinterpret_cast<const uint4*>(d + i * kDescSize);
    uint32_t s2 = 0, s1 = 0;
#pragma unroll
    for (int c = 0; c < kDescSize / 16; c++) {
        const uint4 w = p[c];
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t b = (ws[q] >> (8 * j)) & 0xff;
                s2 += b * b;
                s1 += b;
            }
    }
    nrm[i] = (int)s2 - 256 * (int)s1;
}

// (256, 3): with three waves per SIMD asked for, the accumulators stay in the
// VGPRs (119 registers, no AGPR copy, no scratch) and four waves fit; the
// kernel is bound by load latency and the epilogue's VALU issue, which they
// hide: 9.0 -> 6.8 ms on 127 pairs of 8.5 k x 8.5 k rows (profiles/match_pairs.md)
__global__ __launch_bounds__(256, 3) void k_match_seg_tiles(const uint8_t* __restrict__ d,
                                                         const int* __restrict__ nrm,
                                                         const MatchPair* __restrict__ pairs, int n_pairs,
                                                         unsigned long long* __restrict__ best,
                                                         unsigned long long* __restrict__ second,
                                                         unsigned long long* __restrict__ col_best) {
    const int pi = pair_of(pairs, n_pairs, blockIdx.x, true);
    const MatchPair P = pairs[pi];
    const int nq = (int)P.nq, nt = (int)P.nt;
    const uint32_t local = blockIdx.x - P.tile0, ntq = (P.nq + 127) / 128;
    const uint8_t* __restrict__ q = d + (size_t)P.qrow0 * kDescSize;
    const uint8_t* __restrict__ t = d + (size_t)P.trow0 * kDescSize;
    const int* __restrict__ qn = nrm + P.qrow0;
    const int* __restrict__ tn = nrm + P.trow0;
    best += P.qoff;
    second += P.qoff;
    col_best += P.toff;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int q0 = (int)(local % ntq) * 128 + (wave >> 1) * 64;  // this wave's 64 query rows
    const int t0 = (int)(local / ntq) * 128 + (wave & 1) * 64;   // and 64 train rows
    // the tile's 128 query-row terms m_q through LDS: every lane needs 32 of them
    __shared__ int s_qn[128];
    if (threadIdx.x < 128) {
        const int qr = (int)(local % ntq) * 128 + (int)threadIdx.x;
        s_qn[threadIdx.x] = qr < nq ? qn[qr] : kBadD2;
    }
    i32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[a][b][e] = 0;
    // k-step s of lane half h takes bytes [64 h + 16 s, + 16) of a row: any
    // assignment of k to (step, half, element) gives the same sums as long as
    // both operands use it, and this one keeps a lane on one half row
#pragma unroll
    for (int s = 0; s < kDescSize / 32; s++) {
        const int k0 = 64 * h + 16 * s;
        i32x4 fa[2], fb[2];
#pragma unroll
        for (int a = 0; a < 2; a++) fa[a] = load_frag_i8(q, q0 + 32 * a + r, nq, k0);
#pragma unroll
        for (int b = 0; b < 2; b++) fb[b] = load_frag_i8(t, t0 + 32 * b + r, nt, k0);
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++)
                acc[a][b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
    __syncthreads();
    // C/D: column (train) = lane & 31, row (query) = (e & 3) + 8 * (e >> 2) + 4 * h
    int tnorm[2];
    int tc[2];
#pragma unroll
    for (int b = 0; b < 2; b++) {
        tc[b] = t0 + 32 * b + r;
        tnorm[b] = (tc[b] < nt ? tn[tc[b]] : kBadD2) + (1 << 22);
    }
    uint32_t colmin[2] = {~0u, ~0u};
    // per 32-row MFMA tile a: this lane's two columns of each of its 16 rows,
    // sorted, then transposed and merged over the 32 lanes of the half -- lane
    // r leaves with row e = r >> 1 merged over the lanes that share r >> 1
    uint32_t rlo[2], rhi[2];
#pragma unroll
    for (int a = 0; a < 2; a++) {
        uint32_t lo[16], hi[16];
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int lr = 32 * a + (e & 3) + 8 * (e >> 2) + 4 * h;  // row within the wave's 64
            const int qnv = s_qn[(wave >> 1) * 64 + lr];
            uint32_t kr[2];
#pragma unroll
            for (int b = 0; b < 2; b++) {
                const uint32_t di = (uint32_t)(qnv + tnorm[b] - 2 * acc[a][b][e]);  // d^2 (< 2^26 with the bad marks)
                kr[b] = (di << 6) | (uint32_t)(32 * b + r);
                colmin[b] = min(colmin[b], (di << 6) | (uint32_t)lr);
            }
            lo[e] = min(kr[0], kr[1]);
            hi[e] = max(kr[0], kr[1]);
        }
        fold_rows<16>(lo, hi, 16, (r & 16) != 0);
        fold_rows<8>(lo, hi, 8, (r & 8) != 0);
        fold_rows<4>(lo, hi, 4, (r & 4) != 0);
        fold_rows<2>(lo, hi, 2, (r & 2) != 0);
        rlo[a] = lo[0];
        rhi[a] = hi[0];
    }
    const uint64_t INF = ~0ull;
    {
        // last step across lane bit 0: even lanes finish tile a = 0, odd lanes a = 1
        const bool up = (r & 1) != 0;
        uint32_t klo = up ? rlo[1] : rlo[0], khi = up ? rhi[1] : rhi[0];
        const uint32_t slo = up ? rlo[0] : rlo[1], shi = up ? rhi[0] : rhi[1];
        merge2(klo, khi, __shfl_xor(slo, 1), __shfl_xor(shi, 1));
        const int e = r >> 1;  // bits 4..1 of the lane chose the row at the four fold steps
        const int qr = q0 + 32 * (r & 1) + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (qr < nq && klo < kBadKey) {
            const uint64_t k1 = ((uint64_t)(klo >> 6) << 32) | (uint32_t)(t0 + (int)(klo & 63));
            const uint64_t old = atomicMin(&best[qr], (unsigned long long)k1);
            const uint64_t loser = old < k1 ? k1 : old;
            if (loser != INF) atomicMin(&second[qr], (unsigned long long)loser);
            if (khi < kBadKey) {
                const uint64_t k2 = ((uint64_t)(khi >> 6) << 32) | (uint32_t)(t0 + (int)(khi & 63));
                atomicMin(&second[qr], (unsigned long long)k2);
            }
        }
    }
    // column minimum over both lane halves
#pragma unroll
    for (int b = 0; b < 2; b++) {
        const uint32_t k = min(colmin[b], (uint32_t)__shfl_xor(colmin[b], 32));
        if (h == 0 && tc[b] < nt && k < kBadKey)
            atomicMin(&col_best[tc[b]], (unsigned long long)(((uint64_t)(k >> 6) << 32) | (uint32_t)(q0 + (int)(k & 63))));
    }
}

// Per (pair, query): cross check as k_match_final, the ratio test
// dist1 < ratio * dist2 (f32, one multiply; ratio == 0: none; no second
// neighbour: rejected), and optionally both neighbours (knnMatch, k = 2).
// The guided matcher (match_guided.hip) runs it with lone_passes (no second
// neighbour: dist2 = +inf, the test passes) and max_distance > 0 (kept only if
// dist1 <= max_distance); 0 / 0 is the unguided rule.
__global__ __launch_bounds__(256) void k_match_seg_final(const MatchPair* __restrict__ pairs, int n_pairs,
                                                         uint32_t n_slots,
                                                         const unsigned long long* __restrict__ best,
                                                         const unsigned long long* __restrict__ second,
                                                         const unsigned long long* __restrict__ col_best,
                                                         int cross_check, float ratio, int* __restrict__ train_idx,
                                                         float* __restrict__ dist, int* __restrict__ nb_idx,
                                                         float* __restrict__ nb_dist, float max_distance,
                                                         int lone_passes) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_slots) return;
    const MatchPair P = pairs[pair_of(pairs, n_pairs, i, false)];
    const int qi = (int)(i - P.qoff);  // query index within its segment
    const uint64_t rb = best[i], sb = second[i];
    const bool has1 = rb != ~0ull, has2 = sb != ~0ull;
    const int t1 = has1 ? (int)(uint32_t)rb : -1, t2 = has2 ? (int)(uint32_t)sb : -1;
    // batchDistL2_8u32f: sqrt((float) int)
    const float d1 = has1 ? sqrtf((float)(uint32_t)(rb >> 32)) : INFINITY;
    const float d2 = has2 ? sqrtf((float)(uint32_t)(sb >> 32)) : INFINITY;
    bool keep = has1;
    if (keep && cross_check) keep = (int)(uint32_t)col_best[P.toff + (uint32_t)t1] == qi;
    if (keep && ratio > 0.0f) keep = (has2 || lone_passes) && d1 < ratio * d2;
    if (keep && max_distance > 0.0f) keep = d1 <= max_distance;
    train_idx[i] = keep ? t1 : -1;
    dist[i] = keep ? d1 : 0.0f;
    if (nb_idx) {
        nb_idx[2 * (size_t)i] = t1;
        nb_idx[2 * (size_t)i + 1] = t2;
        nb_dist[2 * (size_t)i] = d1;
        nb_dist[2 * (size_t)i + 1] = d2;
    }
}

void launch_match_seg_prepare(const uint8_t* d, uint32_t n_slots, uint32_t n_cols, const uint2* norm_blocks,
                              uint32_t n_norm_blocks, int* nrm, unsigned long long* best, unsigned long long* second,
                              unsigned long long* col_best, hipStream_t st) {
    (void)hipMemsetAsync(best, 0xff, (size_t)n_slots * 8, st);
    (void)hipMemsetAsync(second, 0xff, (size_t)n_slots * 8, st);
    if (n_cols) (void)hipMemsetAsync(col_best, 0xff, (size_t)n_cols * 8, st);
    if (n_norm_blocks)
        hipLaunchKernelGGL(k_match_seg_norms, dim3(n_norm_blocks), dim3(256), 0, st, d, norm_blocks, nrm);
}

void launch_match_seg_final(const MatchPair* pairs, int n_pairs, uint32_t n_slots, const unsigned long long* best,
                            const unsigned long long* second, const unsigned long long* col_best, int cross_check,
                            float ratio, float max_distance, int lone_passes, int* train_idx, float* dist, int* nb_idx,
                            float* nb_dist, hipStream_t st) {
    hipLaunchKernelGGL(k_match_seg_final, dim3((n_slots + 255) / 256), dim3(256), 0, st, pairs, n_pairs, n_slots, best,
                       second, col_best, cross_check, ratio, train_idx, dist, nb_idx, nb_dist, max_distance,
                       lone_passes);
}

void launch_match_pairs(const uint8_t* d, const MatchPair* pairs, int n_pairs, uint32_t n_tiles, uint32_t n_slots,
                        uint32_t n_cols, const uint2* norm_blocks, uint32_t n_norm_blocks, int cross_check,
                        float ratio, int* nrm, unsigned long long* best, unsigned long long* second,
                        unsigned long long* col_best, int* train_idx, float* dist, int* nb_idx, float* nb_dist,
                        hipStream_t st) {
    if (n_slots == 0) return;
    launch_match_seg_prepare(d, n_slots, n_cols, norm_blocks, n_norm_blocks, nrm, best, second, col_best, st);
    if (n_tiles)
        hipLaunchKernelGGL(k_match_seg_tiles, dim3(n_tiles), dim3(256), 0, st, d, nrm, pairs, n_pairs, best, second,
                           col_best);
    launch_match_seg_final(pairs, n_pairs, n_slots, best, second, col_best, cross_check, ratio, 0.0f, 0, train_idx,
                           dist, nb_idx, nb_dist, st);
}

}  // namespace siftmi
