// Device helpers of the segmented matcher's tile kernels: k_match_seg_tiles
// (match.hip) and its guided form (match_guided.hip) share the i8 fragment
// load, the in-wave 32-bit keys and the top-2 row reduction.
#pragma once
#include "sift_common.h"
#include "sift_kernels.h"

namespace siftmi {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// Inside a wave the keys are 32 bits: (d^2 << 6 | the row's / column's index
// within the wave's 64), d^2 < 2^23; an invalid row or column has kBadD2 added
// to its d^2 (through its m), so its keys sort last and are >= kBadKey.
constexpr int kBadD2 = 1 << 24;
constexpr uint32_t kBadKey = (uint32_t)kBadD2 << 6;

// Merge of two sorted key pairs (valid keys are distinct).
__device__ __forceinline__ void merge2(uint32_t& lo, uint32_t& hi, uint32_t olo, uint32_t ohi) {
    const uint32_t big = max(lo, olo);
    lo = min(lo, olo);
    hi = min(big, min(hi, ohi));
}

// One step of the transposing reduction over n rows held per lane: lanes with
// bit m clear keep rows [0, n/2) and send [n/2, n) to lane ^ m, the others the
// reverse; each lane leaves with n/2 rows merged over twice as many lanes.
template <int N>
__device__ __forceinline__ void fold_rows(uint32_t (&lo)[16], uint32_t (&hi)[16], int m, bool up) {
#pragma unroll
    for (int j = 0; j < N / 2; j++) {
        const uint32_t klo = up ? lo[j + N / 2] : lo[j], khi = up ? hi[j + N / 2] : hi[j];
        const uint32_t slo = up ? lo[j] : lo[j + N / 2], shi = up ? hi[j] : hi[j + N / 2];
        lo[j] = klo;
        hi[j] = khi;
        merge2(lo[j], hi[j], __shfl_xor(slo, m), __shfl_xor(shi, m));
    }
}

__device__ __forceinline__ int pair_of(const MatchPair* __restrict__ pairs, int n_pairs, uint32_t v, bool by_tile) {
    // the last pair whose first tile (first query slot) is <= v
    int lo = 0, hi = n_pairs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((by_tile ? pairs[mid].tile0 : pairs[mid].qoff) <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

// 16 consecutive u8 of one descriptor row, biased by -128 -> i8 MFMA fragment
__device__ __forceinline__ i32x4 load_frag_i8(const uint8_t* __restrict__ base, int row, int n, int k0) {
    i32x4 f = {0, 0, 0, 0};
    if (row < n) {
        const uint4 w = *reinterpret_cast<const uint4*>(base + (size_t)row * kDescSize + k0);
        f[0] = (int)(w.x ^ 0x80808080u);
        f[1] = (int)(w.y ^ 0x80808080u);
        f[2] = (int)(w.z ^ 0x80808080u);
        f[3] = (int)(w.w ^ 0x80808080u);
    }
    return f;
}

}  // namespace siftmi
