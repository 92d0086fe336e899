// Geometric verification of matched pairs: RANSAC homography with a
// least-squares refit on the inliers.
//
// LABELLED EXTENSION: the crate has nothing like it (examples/sift-match.rs
// stops at drawing the matches).  tests/verify_ref.py is the definition; the
// kernels follow its operand order, and the library is built with
// -ffp-contract=off, so the sampling (u32), the minimal-sample models (f64),
// the scores (f32) and with them the winning hypothesis and its mask are the
// restatement's bits.  Only the refit's 23 sums are added in another order.
//
//   k_verify_gather   per match its record (x, y, X, Y): everything after it
//                     reads contiguous 16-byte records
//   k_verify_models   one lane per (pair, hypothesis): sample, orientation
//                     test, f64 solve -> 9 f32 (all 0: invalid)
//   k_verify_score    a workgroup = 256 hypotheses of one pair; the pair's
//                     records stream through LDS, every lane reads the same
//                     address (a broadcast); (count << 32 | ~h) folded into
//                     the pair's slot with one 64-bit atomicMax
//   k_verify_finish   one workgroup per pair: the winner's mask, the refit
//                     rounds, the sift_mi_homography record
//
// The *_progressive calls (PROSAC; tests/prosac_ref.py) swap two
// of them and leave the rest:
//
//   k_verify_gather_ranked  the gather, with the pair's records in the order of
//                           their quality and perm[] back to the caller's matches
//   k_verify_models_prog    k_verify_models' body with the progressive sample
//   k_verify_finish         with perm: the mask in the caller's match order
#include "verify_common.h"

namespace siftmi {

namespace {

using vfy::finite9;
using vfy::wave_sum;

__device__ __forceinline__ double area2(double ax, double ay, double bx, double by, double cx, double cy) {
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

__device__ __forceinline__ void adj3(const double (&m)[3][3], double (&a)[3][3]) {
    a[0][0] = m[1][1] * m[2][2] - m[1][2] * m[2][1];
    a[0][1] = m[0][2] * m[2][1] - m[0][1] * m[2][2];
    a[0][2] = m[0][1] * m[1][2] - m[0][2] * m[1][1];
    a[1][0] = m[1][2] * m[2][0] - m[1][0] * m[2][2];
    a[1][1] = m[0][0] * m[2][2] - m[0][2] * m[2][0];
    a[1][2] = m[0][2] * m[1][0] - m[0][0] * m[1][2];
    a[2][0] = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    a[2][1] = m[0][1] * m[2][0] - m[0][0] * m[2][1];
    a[2][2] = m[0][0] * m[1][1] - m[0][1] * m[1][0];
}

// The matrix that sends the projective basis to the four points.
__device__ __forceinline__ void basis3(const double (&px)[4], const double (&py)[4], double (&b)[3][3]) {
    const double m[3][3] = {{px[0], px[1], px[2]}, {py[0], py[1], py[2]}, {1.0, 1.0, 1.0}};
    double a[3][3];
    adj3(m, a);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double lam = (a[c][0] * px[3] + a[c][1] * py[3]) + a[c][2];
#pragma unroll
        for (int r = 0; r < 3; r++) b[r][c] = m[r][c] * lam;
    }
}

__device__ __forceinline__ bool inlier(const float (&h)[9], const float4 r, float t2) {
    const float w = (h[6] * r.x + h[7] * r.y) + h[8];
    const float u = (h[0] * r.x + h[1] * r.y) + h[2];
    const float v = (h[3] * r.x + h[4] * r.y) + h[5];
    const float du = r.z * w - u, dv = r.w * w - v;
    return w > 0.0f && du * du + dv * dv <= t2 * (w * w);
}

struct HomographyModel {
    static constexpr uint32_t kMinMatches = 4;
    static __device__ __forceinline__ bool valid(const float (&h)[9]) { return h[8] == 1.0f; }
    static __device__ __forceinline__ bool inlier(const float (&h)[9], const float4 r, float t2) {
        return siftmi::inlier(h, r, t2);
    }
};

}  // namespace

__global__ __launch_bounds__(256) void k_verify_gather(const OutKp* __restrict__ kps,
                                                       const VerifyMatch* __restrict__ matches,
                                                       const VerifyPair* __restrict__ pairs, int n_pairs,
                                                       uint32_t n_rec, float4* __restrict__ rec) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rec) return;
    // the last pair whose first record is <= i (the host checked every index)
    int lo = 0, hi = n_pairs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pairs[mid].rec0 <= i) lo = mid;
        else hi = mid;
    }
    const VerifyPair P = pairs[lo];
    const VerifyMatch mt = matches[i];
    const OutKp q = kps[(size_t)P.qrow0 + (uint32_t)mt.query_idx];
    const OutKp t = kps[(size_t)P.trow0 + (uint32_t)mt.train_idx];
    rec[i] = make_float4(q.x, q.y, t.x, t.y);
}

// The gather of the progressive calls: a pair's records in rank order.  Match i
// has the key (u32 pattern of its quality << 32 | i), rank_i = #{j of the pair:
// key_j < key_i}; the keys are distinct (the index is in them), so the ranks are
// a permutation and one strict compare is the whole rule.  wgs[b] = (pair, first
// match of workgroup b within it): no workgroup straddles a pair.  Each lane holds
// kRankQ matches; the pair's keys pass through LDS kVerifyRankStage at a time,
// every lane reading the same address (a broadcast), slots past the pair's end
// hold all ones, which is below no key.  A rank is a count: no order of lanes or
// stages can show, there is no atomic, and no lane reads a key outside its pair.
// quality null: the matches' own distance.
constexpr int kRankQ = 2;
static_assert(kVerifyRankRows == 256 * kRankQ, "sift_kernels.h states the matches of a workgroup");
static_assert(kVerifyRankStage % 256 == 0 && kVerifyRankStage % 4 == 0, "staging and the unrolled walk");

__global__ __launch_bounds__(256) void k_verify_gather_ranked(const OutKp* __restrict__ kps,
                                                              const VerifyMatch* __restrict__ matches,
                                                              const VerifyPair* __restrict__ pairs,
                                                              const uint2* __restrict__ wgs,
                                                              const float* __restrict__ quality,
                                                              float4* __restrict__ rec, uint32_t* __restrict__ perm) {
    __shared__ unsigned long long s_key[kVerifyRankStage];
    const uint2 wg = wgs[blockIdx.x];
    const uint32_t t = threadIdx.x;
    const VerifyPair P = pairs[wg.x];
    const auto key_of = [&](uint32_t j) {  // j < P.m
        const float v = quality ? quality[(size_t)P.rec0 + j] : matches[(size_t)P.rec0 + j].distance;
        return ((unsigned long long)__float_as_uint(v) << 32) | j;
    };
    unsigned long long key[kRankQ];
    uint32_t rank[kRankQ];
#pragma unroll
    for (int q = 0; q < kRankQ; q++) {
        const uint32_t i = wg.y + (uint32_t)q * 256u + t;
        key[q] = i < P.m ? key_of(i) : 0ull;  // a lane past the pair's end: nothing is stored
        rank[q] = 0;
    }
    for (uint32_t base = 0; base < P.m; base += kVerifyRankStage) {
        const uint32_t cnt = min((uint32_t)kVerifyRankStage, P.m - base);
        __syncthreads();  // the walk over the previous stage is over
#pragma unroll
        for (uint32_t k = t; k < (uint32_t)kVerifyRankStage; k += 256u) s_key[k] = k < cnt ? key_of(base + k) : ~0ull;
        __syncthreads();
        const uint32_t lim = (cnt + 3u) & ~3u;
#pragma unroll 4
        for (uint32_t k = 0; k < lim; k++) {
            const unsigned long long v = s_key[k];
#pragma unroll
            for (int q = 0; q < kRankQ; q++) rank[q] += v < key[q] ? 1u : 0u;
        }
    }
#pragma unroll
    for (int q = 0; q < kRankQ; q++) {
        const uint32_t i = wg.y + (uint32_t)q * 256u + t;
        if (i >= P.m) continue;
        const VerifyMatch mt = matches[(size_t)P.rec0 + i];
        const OutKp a = kps[(size_t)P.qrow0 + (uint32_t)mt.query_idx];
        const OutKp b = kps[(size_t)P.trow0 + (uint32_t)mt.train_idx];
        rec[(size_t)P.rec0 + rank[q]] = make_float4(a.x, a.y, b.x, b.y);
        perm[(size_t)P.rec0 + rank[q]] = i;
    }
}

// kProgressive: the sample comes from the growth table's slice of the pair
// (vfy::sample_progressive) over records in rank order; a compile-time choice,
// so the uniform kernel's code is what it was.
template <bool kProgressive>
__device__ __forceinline__ void models_body(const float4* __restrict__ rec, const VerifyPair* __restrict__ pairs,
                                            const uint32_t* __restrict__ growth, uint32_t seed, uint32_t iterations,
                                            uint32_t blocks_per_pair, float* __restrict__ models) {
    const uint32_t p = blockIdx.x / blocks_per_pair;
    const uint32_t h = (blockIdx.x % blocks_per_pair) * 256u + threadIdx.x;
    const VerifyPair P = pairs[p];
    if (h >= iterations || P.m < 4) return;
    uint32_t pick[4];
    if constexpr (kProgressive) vfy::sample_progressive<4>(seed, h, P.m, growth + P.rec0, pick);
    else vfy::sample_distinct<4>(seed, h, P.m, pick);
    double x[4], y[4], X[4], Y[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float4 r = rec[(size_t)P.rec0 + pick[k]];
        x[k] = (double)r.x;
        y[k] = (double)r.y;
        X[k] = (double)r.z;
        Y[k] = (double)r.w;
    }
    bool valid = true;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int a = t < 3 ? 0 : 1, b = t < 2 ? 1 : 2, c = t < 1 ? 2 : 3;  // (0,1,2) (0,1,3) (0,2,3) (1,2,3)
        const double sq = area2(x[a], y[a], x[b], y[b], x[c], y[c]);
        const double st = area2(X[a], Y[a], X[b], Y[b], X[c], Y[c]);
        valid = valid && sq != 0.0 && st != 0.0 && ((sq > 0.0) == (st > 0.0));
    }
    double A[3][3], B[3][3], adjA[3][3];
    basis3(x, y, A);
    basis3(X, Y, B);
    adj3(A, adjA);
    double H[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) H[r][c] = (B[r][0] * adjA[0][c] + B[r][1] * adjA[1][c]) + B[r][2] * adjA[2][c];
    float hf[9];
#pragma unroll
    for (int k = 0; k < 9; k++) hf[k] = (float)(H[k / 3][k % 3] / H[2][2]);
    valid = valid && finite9(hf);
    float* out = models + ((size_t)p * iterations + h) * 9;
#pragma unroll
    for (int k = 0; k < 9; k++) out[k] = valid ? hf[k] : 0.0f;
}

__global__ __launch_bounds__(256) void k_verify_models(const float4* __restrict__ rec,
                                                       const VerifyPair* __restrict__ pairs, uint32_t seed,
                                                       uint32_t iterations, uint32_t blocks_per_pair,
                                                       float* __restrict__ models) {
    models_body<false>(rec, pairs, nullptr, seed, iterations, blocks_per_pair, models);
}

__global__ __launch_bounds__(256) void k_verify_models_prog(const float4* __restrict__ rec,
                                                            const VerifyPair* __restrict__ pairs,
                                                            const uint32_t* __restrict__ growth, uint32_t seed,
                                                            uint32_t iterations, uint32_t blocks_per_pair,
                                                            float* __restrict__ models) {
    models_body<true>(rec, pairs, growth, seed, iterations, blocks_per_pair, models);
}

__global__ __launch_bounds__(256) void k_verify_score(const float4* __restrict__ rec,
                                                      const VerifyPair* __restrict__ pairs,
                                                      const float* __restrict__ models, uint32_t iterations,
                                                      uint32_t blocks_per_pair, float thr,
                                                      unsigned long long* __restrict__ best) {
    __shared__ float4 s_rec[kVerifyChunk];
    __shared__ unsigned long long s_key[4];
    vfy::score_body<HomographyModel>(rec, pairs, models, iterations, blocks_per_pair, thr, best, s_rec, s_key);
}

constexpr int kVerifySums = 23;

__global__ __launch_bounds__(256) void k_verify_finish(const float4* __restrict__ rec,
                                                       const VerifyPair* __restrict__ pairs,
                                                       const float* __restrict__ models, uint32_t iterations,
                                                       float thr, uint32_t refit_rounds,
                                                       const unsigned long long* __restrict__ best,
                                                       VerifyModel* __restrict__ out, uint8_t* __restrict__ inliers,
                                                       const uint32_t* __restrict__ perm) {
    __shared__ float s_box[4][8];
    __shared__ double s_sum[4][kVerifySums];
    __shared__ double s_A[8][9];
    __shared__ float s_h[9];
    __shared__ int s_ok, s_cnt[4], s_chg[4];
    const uint32_t p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const VerifyPair P = pairs[p];
    const uint64_t key = best[p];
    const float4* __restrict__ r = rec + P.rec0;
    uint8_t* __restrict__ mask = inliers + P.rec0;
    // the mask byte of record i: with perm (records in rank order) the caller's match perm[i]
    const uint32_t* __restrict__ pm = perm ? perm + P.rec0 : nullptr;
    const auto at = [pm](uint32_t i) { return pm ? pm[i] : i; };
    if (P.m < 4 || key == 0) {  // no model
        for (uint32_t i = tid; i < P.m; i += 256u) mask[at(i)] = 0;
        if (tid == 0) {
            VerifyModel o;
#pragma unroll
            for (int k = 0; k < 9; k++) o.h[k] = 0.0f;
            o.n_matches = P.m;
            o.n_inliers = 0;
            o.best_hypothesis = -1;
            o.refits = 0;
            out[p] = o;
        }
        return;
    }
    const uint32_t bh = ~(uint32_t)key;
    uint32_t n_in = (uint32_t)(key >> 32), refits = 0;
    const float t2 = thr * thr;
    float h[9];
#pragma unroll
    for (int k = 0; k < 9; k++) h[k] = models[((size_t)p * iterations + bh) * 9 + k];
    // lane tid owns matches tid, tid + 256, ...: it alone reads and writes their mask bytes
    for (uint32_t i = tid; i < P.m; i += 256u) mask[at(i)] = inlier(h, r[i], t2) ? 1 : 0;

    if (refit_rounds) {
        // box normalisation over all the pair's matches: min / max are exact in any order
        float lo[4] = {INFINITY, INFINITY, INFINITY, INFINITY}, hi[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (uint32_t i = tid; i < P.m; i += 256u) {
            const float4 v = r[i];
            const float c[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                lo[k] = fminf(lo[k], c[k]);
                hi[k] = fmaxf(hi[k], c[k]);
            }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                lo[k] = fminf(lo[k], __shfl_xor(lo[k], s));
                hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], s));
            }
        if (lane == 0)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                s_box[wave][k] = lo[k];
                s_box[wave][4 + k] = hi[k];
            }
        __syncthreads();
        double dlo[4], dhi[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            dlo[k] = (double)fminf(fminf(s_box[0][k], s_box[1][k]), fminf(s_box[2][k], s_box[3][k]));
            dhi[k] = (double)fmaxf(fmaxf(s_box[0][4 + k], s_box[1][4 + k]), fmaxf(s_box[2][4 + k], s_box[3][4 + k]));
        }
        const double cx = (dlo[0] + dhi[0]) / 2.0, cy = (dlo[1] + dhi[1]) / 2.0;
        const double CX = (dlo[2] + dhi[2]) / 2.0, CY = (dlo[3] + dhi[3]) / 2.0;
        const double sq = 2.0 / fmax(fmax(dhi[0] - dlo[0], dhi[1] - dlo[1]), 1.0);
        const double st = 2.0 / fmax(fmax(dhi[2] - dlo[2], dhi[3] - dlo[3]), 1.0);

        for (uint32_t round = 0; round < refit_rounds; round++) {
            // the 23 distinct sums of the normal equations (verify_ref.SUMS, in that order)
            double S[kVerifySums];
#pragma unroll
            for (int k = 0; k < kVerifySums; k++) S[k] = 0.0;
            for (uint32_t i = tid; i < P.m; i += 256u) {
                if (!mask[at(i)]) continue;
                const float4 v = r[i];
                const double x = ((double)v.x - cx) * sq, y = ((double)v.y - cy) * sq;
                const double X = ((double)v.z - CX) * st, Y = ((double)v.w - CY) * st;
                const double Xx = X * x, Xy = X * y, Yx = Y * x, Yy = Y * y;
                const double R = X * X + Y * Y;
                const double Rx = R * x, Ry = R * y;
                const double t[kVerifySums] = {1.0, x, y, x * x, x * y, y * y, X, Y, Xx, Xy, Yx, Yy,
                                               Xx * x, Xx * y, Xy * y, Yx * x, Yx * y, Yy * y,
                                               Rx, Ry, Rx * x, Rx * y, Ry * y};
#pragma unroll
                for (int k = 0; k < kVerifySums; k++) S[k] += t[k];
            }
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1)
#pragma unroll
                for (int k = 0; k < kVerifySums; k++) S[k] += __shfl_xor(S[k], s);
            if (lane == 0)
#pragma unroll
                for (int k = 0; k < kVerifySums; k++) s_sum[wave][k] = S[k];
            __syncthreads();
            if (tid == 0) {
                double T[kVerifySums];
#pragma unroll
                for (int k = 0; k < kVerifySums; k++) T[k] = ((s_sum[0][k] + s_sum[1][k]) + s_sum[2][k]) + s_sum[3][k];
                const double n = T[0], sx = T[1], sy = T[2], xx = T[3], xy = T[4], yy = T[5], sX = T[6], sY = T[7];
                const double Xx = T[8], Xy = T[9], Yx = T[10], Yy = T[11], Xxx = T[12], Xxy = T[13], Xyy = T[14];
                const double Yxx = T[15], Yxy = T[16], Yyy = T[17], Rx = T[18], Ry = T[19], Rxx = T[20], Rxy = T[21];
                const double Ryy = T[22];
                const double A[8][9] = {{xx, xy, sx, 0, 0, 0, -Xxx, -Xxy, Xx},  {xy, yy, sy, 0, 0, 0, -Xxy, -Xyy, Xy},
                                        {sx, sy, n, 0, 0, 0, -Xx, -Xy, sX},     {0, 0, 0, xx, xy, sx, -Yxx, -Yxy, Yx},
                                        {0, 0, 0, xy, yy, sy, -Yxy, -Yyy, Yy},  {0, 0, 0, sx, sy, n, -Yx, -Yy, sY},
                                        {-Xxx, -Xxy, -Xx, -Yxx, -Yxy, -Yx, Rxx, Rxy, -Rx},
                                        {-Xxy, -Xyy, -Xy, -Yxy, -Yyy, -Yy, Rxy, Ryy, -Ry}};
#pragma unroll
                for (int a = 0; a < 8; a++)
#pragma unroll
                    for (int b = 0; b < 9; b++) s_A[a][b] = A[a][b];
                // Gaussian elimination, partial pivoting (the first largest |pivot|), in LDS
                for (int k = 0; k < 8; k++) {
                    int pv = k;
                    for (int a = k + 1; a < 8; a++)
                        if (fabs(s_A[a][k]) > fabs(s_A[pv][k])) pv = a;
                    if (pv != k)
                        for (int b = 0; b < 9; b++) {
                            const double t = s_A[k][b];
                            s_A[k][b] = s_A[pv][b];
                            s_A[pv][b] = t;
                        }
                    for (int a = k + 1; a < 8; a++) {
                        const double f = s_A[a][k] / s_A[k][k];
                        for (int b = k + 1; b < 9; b++) s_A[a][b] = s_A[a][b] - f * s_A[k][b];
                    }
                }
                double g[8];
#pragma unroll
                for (int k = 7; k >= 0; k--) {
                    double s = s_A[k][8];
#pragma unroll
                    for (int b = k + 1; b < 8; b++) s = s - s_A[k][b] * g[b];
                    g[k] = s / s_A[k][k];
                }
                // H = T_t^-1 G T_q
                double G[3][3];
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    const double g0 = g[3 * a] * sq, g1 = a < 2 ? g[3 * a + 1] * sq : g[7] * sq;
                    const double g2 = a < 2 ? g[3 * a + 2] : 1.0;
                    G[a][0] = g0;
                    G[a][1] = g1;
                    G[a][2] = g2 - (g0 * cx + g1 * cy);
                }
                double H[3][3];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    H[0][c] = G[0][c] / st + CX * G[2][c];
                    H[1][c] = G[1][c] / st + CY * G[2][c];
                    H[2][c] = G[2][c];
                }
                float hf[9];
#pragma unroll
                for (int k = 0; k < 9; k++) hf[k] = (float)(H[k / 3][k % 3] / H[2][2]);
#pragma unroll
                for (int k = 0; k < 9; k++) s_h[k] = hf[k];
                s_ok = finite9(hf) ? 1 : 0;
            }
            __syncthreads();
            if (!s_ok) break;  // uniform
            float h2[9];
#pragma unroll
            for (int k = 0; k < 9; k++) h2[k] = s_h[k];
            int cnt = 0, chg = 0;
            for (uint32_t i = tid; i < P.m; i += 256u) {
                const int in = inlier(h2, r[i], t2) ? 1 : 0;
                cnt += in;
                chg += in != (int)mask[at(i)];
            }
            cnt = wave_sum(cnt);
            chg = wave_sum(chg);
            if (lane == 0) {
                s_cnt[wave] = cnt;
                s_chg[wave] = chg;
            }
            __syncthreads();
            const uint32_t n2 = (uint32_t)(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
            const bool changed = (s_chg[0] + s_chg[1] + s_chg[2] + s_chg[3]) != 0;
            __syncthreads();  // s_cnt / s_chg / s_h / s_sum are rewritten by the next round
            if (n2 < n_in) break;  // rejected: the count dropped
            for (uint32_t i = tid; i < P.m; i += 256u) mask[at(i)] = inlier(h2, r[i], t2) ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 9; k++) h[k] = h2[k];
            n_in = n2;
            refits++;
            if (!changed) break;
        }
    }
    if (tid == 0) {
        VerifyModel o;
#pragma unroll
        for (int k = 0; k < 9; k++) o.h[k] = h[k];
        o.n_matches = P.m;
        o.n_inliers = n_in;
        o.best_hypothesis = (int32_t)bh;
        o.refits = refits;
        out[p] = o;
    }
}

void launch_verify_gather(const OutKp* kps, const VerifyMatch* matches, const VerifyPair* pairs, int n_pairs,
                          uint32_t n_rec, float4* rec, hipStream_t st) {
    hipLaunchKernelGGL(k_verify_gather, dim3((n_rec + 255u) / 256u), dim3(256), 0, st, kps, matches, pairs, n_pairs,
                       n_rec, rec);
}

void launch_verify_gather_ranked(const OutKp* kps, const VerifyMatch* matches, const VerifyPair* pairs,
                                 const VerifyProgressive& prog, float4* rec, hipStream_t st) {
    hipLaunchKernelGGL(k_verify_gather_ranked, dim3(prog.n_wgs), dim3(256), 0, st, kps, matches, pairs, prog.wgs,
                       prog.quality, rec, prog.perm);
}

void launch_verify(const OutKp* kps, const VerifyMatch* matches, const VerifyPair* pairs, int n_pairs, uint32_t n_rec,
                   float thr, uint32_t iterations, uint32_t seed, uint32_t refit_rounds, float4* rec, float* models,
                   unsigned long long* best, VerifyModel* out, uint8_t* inliers, hipStream_t st,
                   const VerifyProgressive* prog) {
    if (n_pairs <= 0) return;
    const uint32_t bpp = (iterations + 255u) / 256u;
    (void)hipMemsetAsync(best, 0, (size_t)n_pairs * 8, st);
    if (n_rec) {
        if (prog) {
            launch_verify_gather_ranked(kps, matches, pairs, *prog, rec, st);
            hipLaunchKernelGGL(k_verify_models_prog, dim3((uint32_t)n_pairs * bpp), dim3(256), 0, st, rec, pairs,
                               prog->growth, seed, iterations, bpp, models);
        } else {
            launch_verify_gather(kps, matches, pairs, n_pairs, n_rec, rec, st);
            hipLaunchKernelGGL(k_verify_models, dim3((uint32_t)n_pairs * bpp), dim3(256), 0, st, rec, pairs, seed,
                               iterations, bpp, models);
        }
        hipLaunchKernelGGL(k_verify_score, dim3((uint32_t)n_pairs * bpp), dim3(256), 0, st, rec, pairs, models,
                           iterations, bpp, thr, best);
    }
    hipLaunchKernelGGL(k_verify_finish, dim3((uint32_t)n_pairs), dim3(256), 0, st, rec, pairs, models, iterations, thr,
                       refit_rounds, best, out, inliers, (const uint32_t*)(prog && n_rec ? prog->perm : nullptr));
}

}  // namespace siftmi
