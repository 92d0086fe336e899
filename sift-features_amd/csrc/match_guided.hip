// Guided matching: the segmented 2-NN matcher of match.hip over the
// (query, train) elements a pair's verified model admits.
//
// LABELLED EXTENSION like the verification it follows.  tests/guided_ref.py
// is the definition: element (i, j) of a pair is admissible when the
// verification's own inlier test holds for the record (x_i, y_i, X_j, Y_j)
// under the pair's model g and t2 = thr * thr -- inlier() of verify.hip for a
// homography, FundamentalModel::inlier of verify_epipolar.hip for a
// fundamental matrix -- and nearest / second / cross check / ratio test are
// the unguided matcher's over the admissible elements only.  A query with one
// admissible candidate has no second neighbour and PASSES the ratio test
// (dist2 = +inf; the unguided rule rejects it), and max_distance > 0 keeps a
// query only if dist1 <= max_distance.
//
// Both inlier tests split into a per-query part, a per-train part and a few
// operations per element; the parts are the tests' own subexpressions in
// their own order, and the library is built with -ffp-contract=off, so the
// gate has the verification's bits:
//   homography   query (u, v, w, lim), lim = t2 (w w) where w > 0 and -1
//                elsewhere (du du + dv dv is >= 0 or NaN, never <= -1);
//                train (X, Y); du = X w - u, dv = Y w - v,
//                admissible iff du du + dv dv <= lim
//   fundamental  query (l0, l1, l2, l0 l0 + l1 l1); train (X, Y, m0 m0 + m1 m1);
//                e = (X l0 + Y l1) + l2, d = qa + tb,
//                admissible iff d > 0 and e e <= t2 d
// A model of nine zeros (the verification's "no model") admits nothing.
//
//   k_guide_terms             the two parts, once per (pair, query) slot and
//                             once per (pair, train) column
//   k_match_seg_tiles_guided  k_match_seg_tiles' tiling and reduction; the gate
//                             runs first, into a per-lane mask of the lane's 64
//                             elements.  A wave whose 64 x 64 block admits
//                             nothing leaves before its loads and MFMAs (the
//                             cull; the branch is wave-uniform and behind the
//                             kernel's only barrier); otherwise an inadmissible
//                             element has kBadD2 added to its d^2, like a row
//                             or column past its segment, and the fold /
//                             atomicMin protocol is match.hip's unchanged
//   k_guide_count             the culled waves of the call (a diagnostic)
//   k_match_seg_final         match.hip's, with lone_passes and max_distance
#include "match_common.h"

namespace siftmi {

namespace {

// d^2 < 2^23 plus the three bad marks (row, column, gate) still leaves
// (d^2 << 6 | index) in 32 bits
static_assert(3ll * kBadD2 + (1ll << 23) < (1ll << 26), "in-wave keys are (d^2 << 6 | index) in 32 bits");

struct HomographyGate {
    static __device__ __forceinline__ float4 query(const float (&h)[9], float x, float y, float t2) {
        const float w = (h[6] * x + h[7] * y) + h[8];
        const float u = (h[0] * x + h[1] * y) + h[2];
        const float v = (h[3] * x + h[4] * y) + h[5];
        return make_float4(u, v, w, w > 0.0f ? t2 * (w * w) : -1.0f);
    }
    static __device__ __forceinline__ float4 train(const float (&)[9], float X, float Y) {
        return make_float4(X, Y, 0.0f, 0.0f);
    }
    static __device__ __forceinline__ float4 no_query() { return make_float4(0.0f, 0.0f, 0.0f, -1.0f); }
    static __device__ __forceinline__ bool admissible(const float4 q, float X, float Y, float, float) {
        const float du = X * q.z - q.x, dv = Y * q.z - q.y;
        return du * du + dv * dv <= q.w;
    }
};

struct FundamentalGate {
    static __device__ __forceinline__ float4 query(const float (&f)[9], float x, float y, float) {
        const float l0 = (f[0] * x + f[1] * y) + f[2];
        const float l1 = (f[3] * x + f[4] * y) + f[5];
        const float l2 = (f[6] * x + f[7] * y) + f[8];
        return make_float4(l0, l1, l2, l0 * l0 + l1 * l1);
    }
    static __device__ __forceinline__ float4 train(const float (&f)[9], float X, float Y) {
        const float m0 = (f[0] * X + f[3] * Y) + f[6];
        const float m1 = (f[1] * X + f[4] * Y) + f[7];
        return make_float4(X, Y, m0 * m0 + m1 * m1, 0.0f);
    }
    static __device__ __forceinline__ float4 no_query() { return make_float4(NAN, NAN, NAN, NAN); }
    static __device__ __forceinline__ bool admissible(const float4 q, float X, float Y, float tb, float t2) {
        const float e = (X * q.x + Y * q.y) + q.z;
        const float d = q.w + tb;
        return d > 0.0f && e * e <= t2 * d;
    }
};

// the last pair whose first train column is <= v
__device__ __forceinline__ int pair_of_col(const MatchPair* __restrict__ pairs, int n_pairs, uint32_t v) {
    int lo = 0, hi = n_pairs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pairs[mid].toff <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace

template <class Gate>
__global__ __launch_bounds__(256) void k_guide_terms(const OutKp* __restrict__ kps,
                                                     const MatchPair* __restrict__ pairs, int n_pairs,
                                                     const float* __restrict__ models, uint32_t n_slots,
                                                     uint32_t n_cols, float thr, float4* __restrict__ qterm,
                                                     float4* __restrict__ tterm) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_slots + n_cols) return;
    const bool is_q = i < n_slots;
    const uint32_t v = is_q ? i : i - n_slots;
    const int pi = is_q ? pair_of(pairs, n_pairs, v, false) : pair_of_col(pairs, n_pairs, v);
    const MatchPair P = pairs[pi];
    float g[9];
#pragma unroll
    for (int k = 0; k < 9; k++) g[k] = models[(size_t)pi * 9 + k];
    const OutKp kp = kps[is_q ? P.qrow0 + (v - P.qoff) : P.trow0 + (v - P.toff)];
    if (is_q) qterm[v] = Gate::query(g, kp.x, kp.y, thr * thr);
    else tterm[v] = Gate::train(g, kp.x, kp.y);
}

// (256, 3) as k_match_seg_tiles; the registers and the scratch use (none) of
// both instances are recorded in profiles/guided_match.md
template <class Gate>
__global__ __launch_bounds__(256, 3) void k_match_seg_tiles_guided(
    const uint8_t* __restrict__ d, const int* __restrict__ nrm, const float4* __restrict__ qterm,
    const float4* __restrict__ tterm, const MatchPair* __restrict__ pairs, int n_pairs, float thr, int cull,
    unsigned long long* __restrict__ best, unsigned long long* __restrict__ second,
    unsigned long long* __restrict__ col_best, uint8_t* __restrict__ culled) {
    const int pi = pair_of(pairs, n_pairs, blockIdx.x, true);
    const MatchPair P = pairs[pi];
    const int nq = (int)P.nq, nt = (int)P.nt;
    const uint32_t local = blockIdx.x - P.tile0, ntq = (P.nq + 127) / 128;
    const uint8_t* __restrict__ q = d + (size_t)P.qrow0 * kDescSize;
    const uint8_t* __restrict__ t = d + (size_t)P.trow0 * kDescSize;
    const int* __restrict__ qn = nrm + P.qrow0;
    const int* __restrict__ tn = nrm + P.trow0;
    qterm += P.qoff;
    tterm += P.toff;
    best += P.qoff;
    second += P.qoff;
    col_best += P.toff;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int q0 = (int)(local % ntq) * 128 + (wave >> 1) * 64;  // this wave's 64 query rows
    const int t0 = (int)(local / ntq) * 128 + (wave & 1) * 64;   // and 64 train rows
    // the tile's 128 query-row terms m_q and gate terms through LDS: every lane needs 32 of each
    __shared__ int s_qn[128];
    __shared__ float4 s_qt[128];
    {
        const int row = (int)threadIdx.x & 127, qr = (int)(local % ntq) * 128 + row;
        if (threadIdx.x < 128) s_qn[row] = qr < nq ? qn[qr] : kBadD2;
        else s_qt[row] = qr < nq ? qterm[qr] : Gate::no_query();
    }
    int tc[2];
    float tX[2], tY[2], tB[2];
#pragma unroll
    for (int b = 0; b < 2; b++) {
        tc[b] = t0 + 32 * b + r;
        // a column past the segment: X = NaN fails either test
        const float4 tt = tc[b] < nt ? tterm[tc[b]] : make_float4(NAN, NAN, NAN, NAN);
        tX[b] = tt.x;
        tY[b] = tt.y;
        tB[b] = tt.z;
    }
    __syncthreads();  // the kernel's only barrier: nothing below it is reached by every wave
    // the gate: bit 2 e + b of adm[a] <-> accumulator element acc[a][b][e]
    const float t2 = thr * thr;
    uint32_t adm[2] = {0u, 0u};
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const float4 qt = s_qt[(wave >> 1) * 64 + 32 * a + (e & 3) + 8 * (e >> 2) + 4 * h];
#pragma unroll
            for (int b = 0; b < 2; b++)
                adm[a] |= Gate::admissible(qt, tX[b], tY[b], tB[b], t2) ? 1u << (2 * e + b) : 0u;
        }
    // the mask lives in two VGPRs: without this the compiler keeps the 64 comparison results as 64
    // lane masks in SGPR pairs across the MFMAs and spills
    asm volatile("" : "+v"(adm[0]), "+v"(adm[1]));
    if (cull && __ballot((adm[0] | adm[1]) != 0u) == 0ull) {  // wave-uniform
        if (lane == 0) culled[4 * (size_t)blockIdx.x + wave] = 1;
        return;
    }

    i32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[a][b][e] = 0;
    // k-step s of lane half h takes bytes [64 h + 16 s, + 16) of a row, as in k_match_seg_tiles
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
    // C/D: column (train) = lane & 31, row (query) = (e & 3) + 8 * (e >> 2) + 4 * h
    int tnorm[2];
#pragma unroll
    for (int b = 0; b < 2; b++) tnorm[b] = (tc[b] < nt ? tn[tc[b]] : kBadD2) + (1 << 22);
    uint32_t colmin[2] = {~0u, ~0u};
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
                const uint32_t bad = (adm[a] >> (2 * e + b)) & 1u ? 0u : (uint32_t)kBadD2;
                const uint32_t di = (uint32_t)(qnv + tnorm[b] - 2 * acc[a][b][e]) + bad;  // < 2^26 with the bad marks
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
        const int e = r >> 1;
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

// culled[4 * tile + wave] is 1 where that wave left at the cull: their sum
__global__ __launch_bounds__(256) void k_guide_count(const uint32_t* __restrict__ culled, uint32_t n_tiles,
                                                     unsigned long long* __restrict__ n_culled) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    int n = i < n_tiles ? __popc(culled[i]) : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) n += __shfl_xor(n, m);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(n_culled, (unsigned long long)n);
}

template <class Gate>
static void launch_guided(const uint8_t* d, const OutKp* kps, const MatchPair* pairs, int n_pairs, uint32_t n_tiles,
                          uint32_t n_slots, uint32_t n_cols, const float* models, float thr, int cull, const int* nrm,
                          unsigned long long* best, unsigned long long* second, unsigned long long* col_best,
                          float4* qterm, float4* tterm, uint32_t* culled, hipStream_t st) {
    hipLaunchKernelGGL(k_guide_terms<Gate>, dim3((n_slots + n_cols + 255u) / 256u), dim3(256), 0, st, kps, pairs,
                       n_pairs, models, n_slots, n_cols, thr, qterm, tterm);
    hipLaunchKernelGGL(k_match_seg_tiles_guided<Gate>, dim3(n_tiles), dim3(256), 0, st, d, nrm, qterm, tterm, pairs,
                       n_pairs, thr, cull, best, second, col_best, reinterpret_cast<uint8_t*>(culled));
}

void launch_match_pairs_guided(const uint8_t* d, const OutKp* kps, const MatchPair* pairs, int n_pairs,
                               uint32_t n_tiles, uint32_t n_slots, uint32_t n_cols, const uint2* norm_blocks,
                               uint32_t n_norm_blocks, bool fundamental, const float* models, float thr, int cull,
                               int cross_check, float ratio, float max_distance, int* nrm, unsigned long long* best,
                               unsigned long long* second, unsigned long long* col_best, float4* qterm, float4* tterm,
                               uint32_t* culled, unsigned long long* n_culled, int* train_idx, float* dist,
                               hipStream_t st) {
    if (n_slots == 0) return;
    launch_match_seg_prepare(d, n_slots, n_cols, norm_blocks, n_norm_blocks, nrm, best, second, col_best, st);
    (void)hipMemsetAsync(n_culled, 0, sizeof(unsigned long long), st);
    if (n_tiles) {
        if (cull) (void)hipMemsetAsync(culled, 0, (size_t)n_tiles * 4, st);
        if (fundamental)
            launch_guided<FundamentalGate>(d, kps, pairs, n_pairs, n_tiles, n_slots, n_cols, models, thr, cull, nrm,
                                           best, second, col_best, qterm, tterm, culled, st);
        else
            launch_guided<HomographyGate>(d, kps, pairs, n_pairs, n_tiles, n_slots, n_cols, models, thr, cull, nrm,
                                          best, second, col_best, qterm, tterm, culled, st);
        if (cull)
            hipLaunchKernelGGL(k_guide_count, dim3((n_tiles + 255u) / 256u), dim3(256), 0, st, culled, n_tiles,
                               n_culled);
    }
    launch_match_seg_final(pairs, n_pairs, n_slots, best, second, col_best, cross_check, ratio, max_distance, 1,
                           train_idx, dist, nullptr, nullptr, st);
}

}  // namespace siftmi
