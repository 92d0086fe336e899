// What the two geometric verifications share (verify.hip: homography,
// verify_epipolar.hip: fundamental matrix): the
// sampling hash, the distinct-index draw, the wave helpers and the scoring
// kernel's body, which only differs in the model's inlier test.
#pragma once
#include "sift_common.h"
#include "sift_kernels.h"

namespace siftmi {
namespace vfy {

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// N distinct indices below m >= N: draw k is uniform over the m - k indices
// not yet picked (stepped over in ascending order), so there is no rejection.
template <int N>
__device__ __forceinline__ void sample_distinct(uint32_t seed, uint32_t h, uint32_t m, uint32_t (&pick)[N]) {
    const uint32_t s = mix32(mix32(seed + 0x9E3779B9u) ^ h);
    uint32_t sorted[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        const uint32_t u = mix32(s + 0x85EBCA6Bu * (uint32_t)(k + 1));
        uint32_t idx = (uint32_t)(((uint64_t)u * (uint64_t)(m - (uint32_t)k)) >> 32);
#pragma unroll
        for (int j = 0; j < k; j++) idx += idx >= sorted[j] ? 1u : 0u;
        pick[k] = idx;
        sorted[k] = idx;
#pragma unroll
        for (int j = k; j > 0; j--) {
            const uint32_t a = sorted[j - 1], b = sorted[j];
            sorted[j - 1] = min(a, b);
            sorted[j] = max(a, b);
        }
    }
}

// The progressive (PROSAC) sample of hypothesis h over a pair's m >= N records
// in rank order (tests/prosac_ref.py).  tab is the pair's slice
// of the growth table (csrc/prosac_growth.h): T'_{i + 1} at position i >= N - 1,
// ascending.  The first position i in [N - 1, m) with h < tab[i] gives n_h = i +
// 1: N - 1 distinct draws below i, then record i as the last member.  Without
// one (the tail, when m is close to N) the uniform draw over all m.
template <int N>
__device__ __forceinline__ void sample_progressive(uint32_t seed, uint32_t h, uint32_t m,
                                                   const uint32_t* __restrict__ tab, uint32_t (&pick)[N]) {
    uint32_t lo = N - 1, hi = m;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (h < tab[mid]) hi = mid;
        else lo = mid + 1;
    }
    if (lo < m) {
        uint32_t head[N - 1];
        sample_distinct<N - 1>(seed, h, lo, head);
#pragma unroll
        for (int k = 0; k < N - 1; k++) pick[k] = head[k];
        pick[N - 1] = lo;
    } else {
        sample_distinct<N>(seed, h, m, pick);
    }
}

__device__ __forceinline__ bool finite9(const float (&h)[9]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; k++) ok = ok && isfinite(h[k]);
    return ok;
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// The scoring kernel's body for a 256-lane workgroup = 256 hypotheses of one
// pair.  Model gives kMinMatches, valid(g) (is the stored model one at all) and
// inlier(g, record, thr * thr).  The pair's records stream through LDS in
// kVerifyChunk pieces, every lane reads the same address (a broadcast), and
// (count << 32 | ~h) is folded into the pair's slot with one 64-bit atomicMax.
template <class Model>
__device__ __forceinline__ void score_body(const float4* __restrict__ rec, const VerifyPair* __restrict__ pairs,
                                           const float* __restrict__ models, uint32_t iterations,
                                           uint32_t blocks_per_pair, float thr,
                                           unsigned long long* __restrict__ best, float4* s_rec,
                                           unsigned long long* s_key) {
    const uint32_t p = blockIdx.x / blocks_per_pair;
    const uint32_t h = (blockIdx.x % blocks_per_pair) * 256u + threadIdx.x;
    const VerifyPair P = pairs[p];
    if (P.m < Model::kMinMatches) return;  // the whole workgroup
    float g[9];
    const bool live = h < iterations;
    const float* src = models + ((size_t)p * iterations + (live ? h : 0u)) * 9;
#pragma unroll
    for (int k = 0; k < 9; k++) g[k] = src[k];
    const bool valid = live && Model::valid(g);  // an invalid sample is stored as zeros
    const float t2 = thr * thr;
    uint32_t cnt = 0;
    for (uint32_t c0 = 0; c0 < P.m; c0 += kVerifyChunk) {
        const uint32_t n = min((uint32_t)kVerifyChunk, P.m - c0);
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < n; j += 256u) s_rec[j] = rec[(size_t)P.rec0 + c0 + j];
        __syncthreads();
#pragma unroll 4
        for (uint32_t j = 0; j < n; j++) cnt += Model::inlier(g, s_rec[j], t2) ? 1u : 0u;
    }
    uint64_t key = valid ? ((uint64_t)cnt << 32) | (uint32_t)~h : 0ull;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const uint64_t o = shfl_xor_u64(key, s);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < 4; w++) key = s_key[w] > key ? s_key[w] : key;
        if (key) atomicMax(&best[p], (unsigned long long)key);
    }
}

}  // namespace vfy
}  // namespace siftmi
