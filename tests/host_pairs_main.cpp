// The host step of the frame-pair proposal (sift-features_amd/csrc/
// pair_propose.h) as a stand-alone program for the sanitizers
// (tests/test_host_pairs.py builds and runs it; nothing is loaded into
// Python).  Input (argv[1]), any number of cases:
//     case NAME N MIN_MATCHES MAX_PARTNERS
//     s_00 s_01 ... (N * N scores, row-major)
// Output per case: "pairs NAME a_0 b_0 a_1 b_1 ..." in the order returned.
#include <cstdint>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "pair_propose.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string tag, name;
    uint32_t n, min_matches, max_partners;
    while (in >> tag >> name >> n >> min_matches >> max_partners) {
        if (tag != "case") return 2;
        // exactly n * n entries on the heap: a read past the matrix is the sanitizer's
        std::vector<uint32_t> sc((size_t)n * n);
        for (uint32_t& v : sc)
            if (!(in >> v)) return 2;
        const std::vector<sift_mi_seg_pair> out = siftmi::propose_from_scores(sc.data(), n, min_matches, max_partners);
        std::cout << "pairs " << name;
        for (const sift_mi_seg_pair& p : out) std::cout << ' ' << p.query_seg << ' ' << p.train_seg;
        std::cout << '\n';
    }
    return 0;
}
