// The host side of the progressive (PROSAC) sampling of the two geometric
// verifications (tests/prosac_ref.py is the definition): the
// growth table a pair's hypotheses bisect, and the check of the qualities its
// matches are ranked by.  Plain C++ without HIP, so the same text builds in a
// stand-alone program (tests/host_prosac_main.cpp).
//
// k is the model's sample size, N the pair's match count, T the call's
// iterations.  All in f64 with one rounding per operation (build without
// contraction): T_k = T, then for i = 0..k-1 T_k = T_k * (k - i) / (N - i);
// T_{n+1} = T_n * (n + 1) / (n + 1 - k); T'_k = 1, T'_{n+1} = T'_n +
// ceil(T_{n+1} - T_n).  Hypothesis h draws from the best n_h matches, n_h the
// smallest n with h < T'_n.  The paper fixes T_N at 200 000 draws; here T_N is
// the call's own iterations, so the schedule reaches the whole set as the call
// ends (a pair of ten matches is not sampled from its top five a thousand
// times).  T_{n+1} - T_n > 0 for every n, so T' ascends strictly, and T'_N <=
// T + N.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace siftmi {
namespace prosac {

// T'_n for n = k, k + 1, ... of one pair, one step at a time (N >= k >= 1).
struct Growth {
    double t;     // T_n
    uint64_t tp;  // T'_n
    uint32_t n, k;
    Growth(uint32_t N, uint32_t k_, uint32_t T) : t((double)T), tp(1), n(k_), k(k_) {
        for (uint32_t i = 0; i < k; i++) {
            t = t * (double)(k - i);
            t = t / (double)(N - i);
        }
    }
    void step() {
        double t1 = t * (double)(n + 1);
        t1 = t1 / (double)(n + 1 - k);
        // ceil of a positive value below 2^32 without the library call: this loop is the call's host cost
        const double d = t1 - t;
        const uint64_t f = (uint64_t)d;
        tp += f + ((double)f < d ? 1u : 0u);
        t = t1;
        n++;
    }
};

// A pair's slice of the device table, one u32 per rank position: T'_{i + 1} at
// position i >= k - 1 (ascending from there on), 0 below.  N < k: all 0, the
// pair has no model.
inline void fill_table(uint32_t N, uint32_t k, uint32_t T, uint32_t* out) {
    for (uint32_t i = 0; i < N && i + 1 < k; i++) out[i] = 0;
    if (N < k) return;
    Growth g(N, k, T);
    out[k - 1] = (uint32_t)g.tp;
    for (uint32_t i = k; i < N; i++) {
        g.step();
        out[i] = (uint32_t)g.tp;
    }
}

// fill_table for the pairs of a call: at(p) gives pair p's match count and the
// first position of its slice in out.  One pair's recurrence is a chain of
// dependent multiplies and divides, so four pairs are stepped in turn over the
// positions they share and each finishes alone: the same steps, the same values.
template <class PairAt>
inline void fill_tables(size_t n_pairs, PairAt at, uint32_t k, uint32_t T, uint32_t* out) {
    constexpr size_t W = 4;
    for (size_t p0 = 0; p0 < n_pairs; p0 += W) {
        uint32_t N[W], live = 0, common = 0xffffffffu;
        uint32_t* o[W];
        Growth g[W] = {Growth(k, k, T), Growth(k, k, T), Growth(k, k, T), Growth(k, k, T)};
        for (size_t j = 0; j < W && p0 + j < n_pairs; j++) {
            uint32_t m, first;
            at(p0 + j, m, first);
            if (m < k) {
                fill_table(m, k, T, out + first);
                continue;
            }
            N[live] = m;
            o[live] = out + first;
            g[live] = Growth(m, k, T);
            for (uint32_t i = 0; i + 1 < k; i++) o[live][i] = 0;
            o[live][k - 1] = 1;
            common = m < common ? m : common;
            live++;
        }
        if (live == W) {
            for (uint32_t i = k; i < common; i++)
                for (size_t j = 0; j < W; j++) {
                    g[j].step();
                    o[j][i] = (uint32_t)g[j].tp;
                }
        } else {
            common = k;
        }
        for (uint32_t j = 0; j < live; j++)
            for (uint32_t i = common; i < N[j]; i++) {
                g[j].step();
                o[j][i] = (uint32_t)g[j].tp;
            }
    }
}

// The u32 pattern of a quality orders as its value iff it is finite with the
// sign bit clear (-0.0 has it set).  0: all n are; 1: one is NaN or infinite;
// 2: one has its sign bit set.  The first offender decides.
inline int check_quality(const float* q, size_t stride_bytes, size_t n) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(q);
    for (size_t i = 0; i < n; i++, p += stride_bytes) {
        uint32_t b;
        std::memcpy(&b, p, 4);
        if ((b & 0x7f800000u) == 0x7f800000u) return 1;
        if (b >> 31) return 2;
    }
    return 0;
}

}  // namespace prosac
}  // namespace siftmi
