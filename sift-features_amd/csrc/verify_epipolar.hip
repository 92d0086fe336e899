// Epipolar verification of matched pairs: RANSAC fundamental matrix from
// 8-point samples, Sampson score, eigen-refit on the inliers.
//
// LABELLED EXTENSION like verify.hip, whose gather kernel, records, sampling
// and scoring structure it reuses.  tests/epipolar_ref.py is the definition;
// the kernels follow its operand order, and the library is built with
// -ffp-contract=off, so the sampling (u32), the box values and the 8-point
// models (f64), the scores (f32) and with them the winning hypothesis and its
// mask are the restatement's bits.  Only the refit's 45 sums are added in
// another order.
//
// (X, Y, 1) F (x, y, 1)^T = 0 for a query point (x, y) and its train point
// (X, Y).  F is the raw 8-point solution (full rank in general) when no refit
// round was accepted, and rank 2 up to its f32 rounding when refits >= 1.
//
//   k_verify_box_f      one workgroup per pair: the six f64 values of the box
//                       normalisation over all the pair's matches
//   k_verify_models_f   one lane per (pair, hypothesis): sample, 8 x 9 f64
//                       system in LDS laid out [entry][lane], Gaussian
//                       elimination with complete pivoting -> 9 f32 (all 0:
//                       invalid)
//   k_verify_score_f    k_verify_score's body with the Sampson inlier test
//   k_verify_finish_f   one workgroup per pair: the winner's mask, the refit
//                       rounds (45 sums, cyclic Jacobi on the 9 x 9 in LDS
//                       spread over nine lanes, rank 2), the sift_mi_fundamental
//                       record
//
// The *_progressive calls (PROSAC; tests/prosac_ref.py) run
// verify.hip's ranking gather in place of its gather, k_verify_models_f_prog
// (this kernel's body with the progressive sample) and k_verify_finish_f with
// perm, which writes the mask in the caller's match order.
#include "verify_common.h"

namespace siftmi {

namespace {

using vfy::finite9;
using vfy::wave_sum;

constexpr int kModelLanes = 64;   // k_verify_models_f's workgroup: 72 doubles per lane in LDS
constexpr int kJacobiSweeps = 10;  // epipolar_ref.SWEEPS

struct FundamentalModel {
    static constexpr uint32_t kMinMatches = 8;
    static __device__ __forceinline__ bool valid(const float (&f)[9]) {
        bool any = false;
#pragma unroll
        for (int k = 0; k < 9; k++) any = any || f[k] != 0.0f;
        return any;
    }
    // Sampson distance <= thr without a division; NaN is never an inlier
    static __device__ __forceinline__ bool inlier(const float (&f)[9], const float4 r, float t2) {
        const float l0 = (f[0] * r.x + f[1] * r.y) + f[2];
        const float l1 = (f[3] * r.x + f[4] * r.y) + f[5];
        const float l2 = (f[6] * r.x + f[7] * r.y) + f[8];
        const float m0 = (f[0] * r.z + f[3] * r.w) + f[6];
        const float m1 = (f[1] * r.z + f[4] * r.w) + f[7];
        const float e = (r.z * l0 + r.w * l1) + l2;
        const float d = (l0 * l0 + l1 * l1) + (m0 * m0 + m1 * m1);
        return d > 0.0f && e * e <= t2 * d;
    }
};

struct Box {
    double cx, cy, sq, CX, CY, st;
};

// F = T_t^T F' T_q, every entry divided by the entry of largest magnitude (the
// first in row-major order on ties), rounded to f32 (epipolar_ref._denorm, _scale_f32).
__device__ __forceinline__ void denorm_scale(const double (&fp)[9], const Box& b, float (&out)[9]) {
    double F[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double g0 = fp[3 * r] * b.sq, g1 = fp[3 * r + 1] * b.sq;
        F[3 * r] = g0;
        F[3 * r + 1] = g1;
        F[3 * r + 2] = fp[3 * r + 2] - (g0 * b.cx + g1 * b.cy);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        F[c] = F[c] * b.st;
        F[3 + c] = F[3 + c] * b.st;
        F[6 + c] = F[6 + c] - (F[c] * b.CX + F[3 + c] * b.CY);
    }
    double big = F[0], mag = fabs(F[0]);
#pragma unroll
    for (int k = 1; k < 9; k++) {
        const double v = fabs(F[k]);
        if (v > mag) {
            mag = v;
            big = F[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 9; k++) out[k] = (float)(F[k] / big);
}

// Cyclic Jacobi on the symmetric n x n matrix a (row stride 9) in LDS; v
// collects the rotations (the caller sets it to the identity).  Called by a
// whole wave: every lane computes the rotation, lane k < n applies it to row k
// of a (and its mirror column) and of v.  The accesses are volatile, so every
// one is made, in program order; a wave's LDS operations complete in order, and
// each rotation reads all it needs before its first write.
__device__ __forceinline__ void jacobi_lds(volatile double* a, volatile double* v, int n, int lane) {
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++)
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                const double apq = a[p * 9 + q];
                if (apq == 0.0) continue;  // the whole wave
                const double app = a[p * 9 + p], aqq = a[q * 9 + q];
                const double theta = (aqq - app) / (2.0 * apq);
                double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                if (lane < n) {
                    const int k = lane;
                    const double akp = a[k * 9 + p], akq = a[k * 9 + q], vkp = v[k * 9 + p], vkq = v[k * 9 + q];
                    if (k != p && k != q) {
                        const double np_ = c * akp - s * akq, nq = s * akp + c * akq;
                        a[k * 9 + p] = np_;
                        a[p * 9 + k] = np_;
                        a[k * 9 + q] = nq;
                        a[q * 9 + k] = nq;
                    } else if (k == p) {
                        a[p * 9 + p] = app - t * apq;
                        a[p * 9 + q] = 0.0;
                        a[q * 9 + p] = 0.0;
                    } else {
                        a[q * 9 + q] = aqq + t * apq;
                    }
                    v[k * 9 + p] = c * vkp - s * vkq;
                    v[k * 9 + q] = s * vkp + c * vkq;
                }
            }
}

// The column of v for the smallest diagonal entry of a (lowest index on ties).
template <int N>
__device__ __forceinline__ void smallest_lds(const volatile double* a, const volatile double* v, double (&out)[N]) {
    int j = 0;
    double w = a[0];
    for (int i = 1; i < N; i++) {
        const double wi = a[i * 9 + i];
        if (wi < w) {
            w = wi;
            j = i;
        }
    }
#pragma unroll
    for (int i = 0; i < N; i++) out[i] = v[i * 9 + j];
}

}  // namespace

__global__ __launch_bounds__(256) void k_verify_box_f(const float4* __restrict__ rec,
                                                      const VerifyPair* __restrict__ pairs,
                                                      double* __restrict__ box) {
    __shared__ float s_box[4][8];
    const uint32_t p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const VerifyPair P = pairs[p];
    if (P.m < 8) return;  // no model: nothing reads the pair's box
    const float4* __restrict__ r = rec + P.rec0;
    // min / max are exact in any order
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
    if (tid != 0) return;
    double dlo[4], dhi[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        dlo[k] = (double)fminf(fminf(s_box[0][k], s_box[1][k]), fminf(s_box[2][k], s_box[3][k]));
        dhi[k] = (double)fmaxf(fmaxf(s_box[0][4 + k], s_box[1][4 + k]), fmaxf(s_box[2][4 + k], s_box[3][4 + k]));
    }
    double* o = box + (size_t)p * 6;
    o[0] = (dlo[0] + dhi[0]) / 2.0;
    o[1] = (dlo[1] + dhi[1]) / 2.0;
    o[2] = 2.0 / fmax(fmax(dhi[0] - dlo[0], dhi[1] - dlo[1]), 1.0);
    o[3] = (dlo[2] + dhi[2]) / 2.0;
    o[4] = (dlo[3] + dhi[3]) / 2.0;
    o[5] = 2.0 / fmax(fmax(dhi[2] - dlo[2], dhi[3] - dlo[3]), 1.0);
}

// kProgressive: the sample comes from the growth table's slice of the pair
// (vfy::sample_progressive) over records in rank order; a compile-time choice,
// so the uniform kernel's code is what it was.
template <bool kProgressive>
__device__ __forceinline__ void models_f_body(const float4* __restrict__ rec, const VerifyPair* __restrict__ pairs,
                                              const double* __restrict__ box, const uint32_t* __restrict__ growth,
                                              uint32_t seed, uint32_t iterations, uint32_t blocks_per_pair,
                                              float* __restrict__ models) {
    // the lane's 8 x 9 system, entry e = 9 r + c at s_a[e][lane]: the bank depends on
    // the lane only, so any per-lane (data-dependent) entry index is conflict-free
    __shared__ double s_a[72][kModelLanes];
    const uint32_t p = blockIdx.x / blocks_per_pair, lane = threadIdx.x;
    const uint32_t h = (blockIdx.x % blocks_per_pair) * (uint32_t)kModelLanes + lane;
    const VerifyPair P = pairs[p];
    if (h >= iterations || P.m < 8) return;  // no barrier below: a lane only touches its own column of s_a
    const double* bp = box + (size_t)p * 6;
    const Box B = {bp[0], bp[1], bp[2], bp[3], bp[4], bp[5]};
#define A_(r, c) s_a[(r) * 9 + (c)][lane]
    uint32_t pick[8];
    if constexpr (kProgressive) vfy::sample_progressive<8>(seed, h, P.m, growth + P.rec0, pick);
    else vfy::sample_distinct<8>(seed, h, P.m, pick);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const float4 v = rec[(size_t)P.rec0 + pick[i]];
        const double x = ((double)v.x - B.cx) * B.sq, y = ((double)v.y - B.cy) * B.sq;
        const double X = ((double)v.z - B.CX) * B.st, Y = ((double)v.w - B.CY) * B.st;
        A_(i, 0) = X * x;
        A_(i, 1) = X * y;
        A_(i, 2) = X;
        A_(i, 3) = Y * x;
        A_(i, 4) = Y * y;
        A_(i, 5) = Y;
        A_(i, 6) = x;
        A_(i, 7) = y;
        A_(i, 8) = 1.0;
    }
    bool valid = true;
    uint64_t perm = 0x876543210ull;  // nibble j: the original column now at position j
#pragma unroll
    for (int k = 0; k < 8; k++) {
        // complete pivoting: the first largest |a[r][c]|, r = k..7, c = k..8, in row-major order
        double bv = fabs(A_(k, k));
        int br = k, bc = k;
#pragma unroll
        for (int r = k; r < 8; r++)
#pragma unroll
            for (int c = k; c < 9; c++) {
                if (r == k && c == k) continue;
                const double v = fabs(A_(r, c));
                if (v > bv) {
                    bv = v;
                    br = r;
                    bc = c;
                }
            }
        valid = valid && bv != 0.0;
        if (br != k) {  // columns < k of these rows are never read again
#pragma unroll
            for (int c = k; c < 9; c++) {
                const double t = A_(k, c);
                A_(k, c) = A_(br, c);
                A_(br, c) = t;
            }
        }
        if (bc != k) {
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const double t = A_(r, k);
                A_(r, k) = A_(r, bc);
                A_(r, bc) = t;
            }
            const uint64_t nk = (perm >> (4 * k)) & 15ull, nc = (perm >> (4 * bc)) & 15ull;
            perm = (perm & ~((15ull << (4 * k)) | (15ull << (4 * bc)))) | (nc << (4 * k)) | (nk << (4 * bc));
        }
        double row[9];
#pragma unroll
        for (int c = k; c < 9; c++) row[c] = A_(k, c);
#pragma unroll
        for (int r = k + 1; r < 8; r++) {
            const double f = A_(r, k) / row[k];
#pragma unroll
            for (int c = k + 1; c < 9; c++) A_(r, c) = A_(r, c) - f * row[c];
        }
    }
    double g[9];
    g[8] = 1.0;
#pragma unroll
    for (int k = 7; k >= 0; k--) {
        double s = -A_(k, 8);
#pragma unroll
        for (int c = k + 1; c < 8; c++) s = s - A_(k, c) * g[c];
        g[k] = s / A_(k, k);
    }
    // undo the column permutation through the lane's LDS column (the system is no longer needed)
#pragma unroll
    for (int j = 0; j < 9; j++) s_a[(perm >> (4 * j)) & 15ull][lane] = g[j];
    double fp[9];
#pragma unroll
    for (int j = 0; j < 9; j++) fp[j] = s_a[j][lane];
#undef A_
    float hf[9];
    denorm_scale(fp, B, hf);
    valid = valid && finite9(hf);
    float* out = models + ((size_t)p * iterations + h) * 9;
#pragma unroll
    for (int k = 0; k < 9; k++) out[k] = valid ? hf[k] : 0.0f;
}

__global__ __launch_bounds__(kModelLanes) void k_verify_models_f(const float4* __restrict__ rec,
                                                                 const VerifyPair* __restrict__ pairs,
                                                                 const double* __restrict__ box, uint32_t seed,
                                                                 uint32_t iterations, uint32_t blocks_per_pair,
                                                                 float* __restrict__ models) {
    models_f_body<false>(rec, pairs, box, nullptr, seed, iterations, blocks_per_pair, models);
}

__global__ __launch_bounds__(kModelLanes) void k_verify_models_f_prog(const float4* __restrict__ rec,
                                                                      const VerifyPair* __restrict__ pairs,
                                                                      const double* __restrict__ box,
                                                                      const uint32_t* __restrict__ growth,
                                                                      uint32_t seed, uint32_t iterations,
                                                                      uint32_t blocks_per_pair,
                                                                      float* __restrict__ models) {
    models_f_body<true>(rec, pairs, box, growth, seed, iterations, blocks_per_pair, models);
}

__global__ __launch_bounds__(256) void k_verify_score_f(const float4* __restrict__ rec,
                                                        const VerifyPair* __restrict__ pairs,
                                                        const float* __restrict__ models, uint32_t iterations,
                                                        uint32_t blocks_per_pair, float thr,
                                                        unsigned long long* __restrict__ best) {
    __shared__ float4 s_rec[kVerifyChunk];
    __shared__ unsigned long long s_key[4];
    vfy::score_body<FundamentalModel>(rec, pairs, models, iterations, blocks_per_pair, thr, best, s_rec, s_key);
}

constexpr int kEpipolarSums = 45;

__global__ __launch_bounds__(256) void k_verify_finish_f(const float4* __restrict__ rec,
                                                         const VerifyPair* __restrict__ pairs,
                                                         const float* __restrict__ models,
                                                         const double* __restrict__ box, uint32_t iterations,
                                                         float thr, uint32_t refit_rounds,
                                                         const unsigned long long* __restrict__ best,
                                                         VerifyModel* __restrict__ out, uint8_t* __restrict__ inliers,
                                                         const uint32_t* __restrict__ perm) {
    __shared__ double s_sum[4][kEpipolarSums];
    __shared__ double s_J[81], s_V[81];
    __shared__ float s_f[9];
    __shared__ int s_ok, s_cnt[4], s_chg[4];
    const uint32_t p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const VerifyPair P = pairs[p];
    const uint64_t key = best[p];
    const float4* __restrict__ r = rec + P.rec0;
    uint8_t* __restrict__ mask = inliers + P.rec0;
    // the mask byte of record i: with perm (records in rank order) the caller's match perm[i]
    const uint32_t* __restrict__ pm = perm ? perm + P.rec0 : nullptr;
    const auto at = [pm](uint32_t i) { return pm ? pm[i] : i; };
    if (P.m < 8 || key == 0) {  // no model
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
    float f[9];
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = models[((size_t)p * iterations + bh) * 9 + k];
    // lane tid owns matches tid, tid + 256, ...: it alone reads and writes their mask bytes
    for (uint32_t i = tid; i < P.m; i += 256u) mask[at(i)] = FundamentalModel::inlier(f, r[i], t2) ? 1 : 0;

    if (refit_rounds) {
        const double* bp = box + (size_t)p * 6;
        const Box B = {bp[0], bp[1], bp[2], bp[3], bp[4], bp[5]};
        for (uint32_t round = 0; round < refit_rounds; round++) {
            if (n_in < 8) break;  // rejected: nothing to fit (uniform)
            // the 45 distinct sums of A^T A (epipolar_ref.SUMS, in that order)
            double S[kEpipolarSums];
#pragma unroll
            for (int k = 0; k < kEpipolarSums; k++) S[k] = 0.0;
            for (uint32_t i = tid; i < P.m; i += 256u) {
                if (!mask[at(i)]) continue;
                const float4 v = r[i];
                const double x = ((double)v.x - B.cx) * B.sq, y = ((double)v.y - B.cy) * B.sq;
                const double X = ((double)v.z - B.CX) * B.st, Y = ((double)v.w - B.CY) * B.st;
                const double t[9] = {X * x, X * y, X, Y * x, Y * y, Y, x, y, 1.0};
                int n = 0;
#pragma unroll
                for (int j = 0; j < 9; j++)
#pragma unroll
                    for (int k = j; k < 9; k++) S[n++] += t[j] * t[k];
            }
            // one sum at a time through the butterfly: few shuffled values live at once
#pragma unroll
            for (int k = 0; k < kEpipolarSums; k++)
#pragma unroll
                for (int s = 32; s >= 1; s >>= 1) S[k] += __shfl_xor(S[k], s);
            if (lane == 0)
#pragma unroll
                for (int k = 0; k < kEpipolarSums; k++) s_sum[wave][k] = S[k];
            __syncthreads();
            if (tid < 81) {
                const int a = min(tid / 9u, tid % 9u), b = max(tid / 9u, tid % 9u);
                const int n = a * 9 - a * (a - 1) / 2 + (b - a);  // (a, b) in the row-by-row upper triangle
                s_J[tid] = ((s_sum[0][n] + s_sum[1][n]) + s_sum[2][n]) + s_sum[3][n];
                s_V[tid] = tid / 9u == tid % 9u ? 1.0 : 0.0;
            }
            __syncthreads();
            if (wave == 0) {
                jacobi_lds(s_J, s_V, 9, (int)lane);
                double fp[9];
                if (lane == 0) {
                    smallest_lds<9>(s_J, s_V, fp);
                    // rank 2: the smallest eigenvector of the 3 x 3 F'^T F'
                    volatile double* J = s_J;
                    volatile double* V = s_V;
#pragma unroll
                    for (int i = 0; i < 3; i++)
#pragma unroll
                        for (int j = 0; j < 3; j++) {
                            J[i * 9 + j] = (fp[i] * fp[j] + fp[3 + i] * fp[3 + j]) + fp[6 + i] * fp[6 + j];
                            V[i * 9 + j] = i == j ? 1.0 : 0.0;
                        }
                }
                jacobi_lds(s_J, s_V, 3, (int)lane);
                if (lane == 0) {
                    double v[3];
                    smallest_lds<3>(s_J, s_V, v);
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        const double fv = (fp[3 * a] * v[0] + fp[3 * a + 1] * v[1]) + fp[3 * a + 2] * v[2];
#pragma unroll
                        for (int c = 0; c < 3; c++) fp[3 * a + c] = fp[3 * a + c] - fv * v[c];
                    }
                    float hf[9];
                    denorm_scale(fp, B, hf);
#pragma unroll
                    for (int k = 0; k < 9; k++) s_f[k] = hf[k];
                    s_ok = finite9(hf) ? 1 : 0;
                }
            }
            __syncthreads();
            if (!s_ok) break;  // uniform
            float f2[9];
#pragma unroll
            for (int k = 0; k < 9; k++) f2[k] = s_f[k];
            int cnt = 0, chg = 0;
            for (uint32_t i = tid; i < P.m; i += 256u) {
                const int in = FundamentalModel::inlier(f2, r[i], t2) ? 1 : 0;
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
            __syncthreads();  // s_cnt / s_chg / s_f / s_sum / s_J are rewritten by the next round
            if (n2 < n_in) break;  // rejected: the count dropped
            for (uint32_t i = tid; i < P.m; i += 256u) mask[at(i)] = FundamentalModel::inlier(f2, r[i], t2) ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 9; k++) f[k] = f2[k];
            n_in = n2;
            refits++;
            if (!changed) break;
        }
    }
    if (tid == 0) {
        VerifyModel o;
#pragma unroll
        for (int k = 0; k < 9; k++) o.h[k] = f[k];
        o.n_matches = P.m;
        o.n_inliers = n_in;
        o.best_hypothesis = (int32_t)bh;
        o.refits = refits;
        out[p] = o;
    }
}

void launch_verify_epipolar(const OutKp* kps, const VerifyMatch* matches, const VerifyPair* pairs, int n_pairs,
                            uint32_t n_rec, float thr, uint32_t iterations, uint32_t seed, uint32_t refit_rounds,
                            float4* rec, double* box, float* models, unsigned long long* best, VerifyModel* out,
                            uint8_t* inliers, hipStream_t st, const VerifyProgressive* prog) {
    if (n_pairs <= 0) return;
    const uint32_t bpp = (iterations + 255u) / 256u, bpp_m = (iterations + kModelLanes - 1u) / kModelLanes;
    (void)hipMemsetAsync(best, 0, (size_t)n_pairs * 8, st);
    if (n_rec) {
        if (prog) launch_verify_gather_ranked(kps, matches, pairs, *prog, rec, st);
        else launch_verify_gather(kps, matches, pairs, n_pairs, n_rec, rec, st);
        hipLaunchKernelGGL(k_verify_box_f, dim3((uint32_t)n_pairs), dim3(256), 0, st, rec, pairs, box);
        if (prog)
            hipLaunchKernelGGL(k_verify_models_f_prog, dim3((uint32_t)n_pairs * bpp_m), dim3(kModelLanes), 0, st, rec,
                               pairs, box, prog->growth, seed, iterations, bpp_m, models);
        else
            hipLaunchKernelGGL(k_verify_models_f, dim3((uint32_t)n_pairs * bpp_m), dim3(kModelLanes), 0, st, rec, pairs,
                               box, seed, iterations, bpp_m, models);
        hipLaunchKernelGGL(k_verify_score_f, dim3((uint32_t)n_pairs * bpp), dim3(256), 0, st, rec, pairs, models,
                           iterations, bpp, thr, best);
    }
    hipLaunchKernelGGL(k_verify_finish_f, dim3((uint32_t)n_pairs), dim3(256), 0, st, rec, pairs, models, box, iterations,
                       thr, refit_rounds, best, out, inliers, (const uint32_t*)(prog && n_rec ? prog->perm : nullptr));
}

}  // namespace siftmi
