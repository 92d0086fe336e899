// The host step of sift_mi_propose_pairs_device: the proposed frame pairs from
// the n x n score matrix (tests/pairs_ref.py, "proposal").  Plain C++ with no
// HIP in it, so that the same text is api.cpp's and a stand-alone program's
// for the sanitizers (tests/host_pairs_main.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/sift_mi.h"

namespace siftmi {

// s(a, b) = max of the two directions; a < b is a candidate when s >=
// min_matches; with max_partners > 0 every frame keeps its first max_partners
// candidates by (s descending, partner ascending) and a pair is proposed when
// either of its frames keeps it.  Sorted by (a, b).
inline std::vector<sift_mi_seg_pair> propose_from_scores(const uint32_t* sc, uint32_t n, uint32_t min_matches,
                                                         uint32_t max_partners) {
    auto s = [&](uint32_t a, uint32_t b) { return std::max(sc[(size_t)a * n + b], sc[(size_t)b * n + a]); };
    std::vector<sift_mi_seg_pair> out;
    if (max_partners == 0) {
        for (uint32_t a = 0; a < n; a++)
            for (uint32_t b = a + 1; b < n; b++)
                if (s(a, b) >= min_matches) out.push_back(sift_mi_seg_pair{a, b});
        return out;
    }
    std::vector<std::pair<uint32_t, uint32_t>> cand;  // (score, partner) of one frame
    for (uint32_t f = 0; f < n; f++) {
        cand.clear();
        for (uint32_t p = 0; p < n; p++)
            if (p != f && s(f, p) >= min_matches) cand.emplace_back(s(f, p), p);
        const size_t k = std::min<size_t>(max_partners, cand.size());
        std::partial_sort(cand.begin(), cand.begin() + k, cand.end(), [](const auto& x, const auto& y) {
            return x.first != y.first ? x.first > y.first : x.second < y.second;
        });
        for (size_t i = 0; i < k; i++) {
            const uint32_t p = cand[i].second;
            out.push_back(sift_mi_seg_pair{std::min(f, p), std::max(f, p)});
        }
    }
    std::sort(out.begin(), out.end(), [](const sift_mi_seg_pair& x, const sift_mi_seg_pair& y) {
        return x.query_seg != y.query_seg ? x.query_seg < y.query_seg : x.train_seg < y.train_seg;
    });
    out.erase(std::unique(out.begin(), out.end(),
                          [](const sift_mi_seg_pair& x, const sift_mi_seg_pair& y) {
                              return x.query_seg == y.query_seg && x.train_seg == y.train_seg;
                          }),
              out.end());
    return out;
}

}  // namespace siftmi
