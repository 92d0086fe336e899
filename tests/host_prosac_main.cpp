// Stand-alone driver of csrc/prosac_growth.h for tests/test_host_prosac.py:
// built with the host compilers under AddressSanitizer and UBSan, no HIP.
//
//   host_prosac tables <file> <n_max>   for k in {4, 8}, T in {1, 255, 1024, 65536}, N = k..n_max:
//                                       fill_table's N u32 appended to <file>, in that order;
//                                       fill_tables against fill_table on mixed pair sizes
//   host_prosac quality                 check_quality on the cases below, one line each
//   host_prosac huge <N> <k> <T>        T'_k, T'_{k+1}, T'_{k+2} and T'_N by stepping (no table)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "prosac_growth.h"

using namespace siftmi::prosac;

static float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "tables")) {
        const uint32_t n_max = (uint32_t)std::atol(argv[3]);
        FILE* f = std::fopen(argv[2], "wb");
        if (!f) return 2;
        const uint32_t Ts[4] = {1, 255, 1024, 65536};
        for (uint32_t k : {4u, 8u})
            for (uint32_t T : Ts)
                for (uint32_t N = k; N <= n_max; N++) {
                    std::vector<uint32_t> tab(N);  // exactly N: a write past the slice is the sanitizer's
                    fill_table(N, k, T, tab.data());
                    if (std::fwrite(tab.data(), 4, N, f) != N) return 3;
                }
        // below k: all zero, nothing past the slice
        for (uint32_t N = 0; N < 8; N++) {
            std::vector<uint32_t> tab(N, 7u);
            fill_table(N, 8, 1024, tab.data());
            for (uint32_t v : tab)
                if (v) return 4;
        }
        // the call's form, four pairs stepped in turn: the same values as one pair at a time
        for (uint32_t k : {4u, 8u}) {
            const uint32_t sizes[] = {0, 300, 7, 1030, 64, 8, 200, 0, 2049, 3, 4, 5, 65, 65, 64, 63, 1025, 9, 12};
            const size_t n = sizeof(sizes) / sizeof(sizes[0]);
            for (size_t n_pairs = 0; n_pairs <= n; n_pairs++) {
                std::vector<uint32_t> first(n_pairs + 1, 0);
                for (size_t p = 0; p < n_pairs; p++) first[p + 1] = first[p] + sizes[p];
                std::vector<uint32_t> all(first[n_pairs], 7u), one(first[n_pairs], 9u);
                fill_tables(n_pairs, [&](size_t p, uint32_t& m, uint32_t& at) { m = sizes[p], at = first[p]; }, k, 1024,
                            all.data());
                for (size_t p = 0; p < n_pairs; p++) fill_table(sizes[p], k, 1024, one.data() + first[p]);
                if (all != one) return 6;
            }
        }
        return std::fclose(f) ? 5 : 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "quality")) {
        struct Match {
            int32_t q, t;
            float d;
        };
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        const float cases[] = {0.0f,  1.0f, 3.5e38f, from_bits(1u) /* the least denormal */,
                               -0.0f, -1.0f, inf,    -inf,
                               nan,   from_bits(0xffc00000u) /* a NaN with the sign bit set */,
                               from_bits(0x7f800001u) /* a signalling NaN */};
        for (float bad : cases) {
            std::vector<float> q(5, 2.0f);
            std::vector<Match> m(5, Match{0, 0, 2.0f});
            q[3] = bad;
            m[3].d = bad;
            uint32_t bits;
            std::memcpy(&bits, &bad, 4);
            std::printf("quality %08x %d %d %d\n", bits, check_quality(q.data(), sizeof(float), q.size()),
                        check_quality(&m[0].d, sizeof(Match), m.size()), check_quality(q.data(), sizeof(float), 3));
        }
        std::printf("quality empty %d\n", check_quality(nullptr, sizeof(float), 0));
        return 0;
    }
    if (argc == 5 && !std::strcmp(argv[1], "huge")) {
        const uint32_t N = (uint32_t)std::strtoul(argv[2], nullptr, 10), k = (uint32_t)std::atol(argv[3]);
        Growth g(N, k, (uint32_t)std::atol(argv[4]));
        std::printf("huge %u %u", N, k);
        for (uint32_t n = k; n < N; n++) {
            if (n < k + 3) std::printf(" %llu", (unsigned long long)g.tp);
            g.step();
        }
        std::printf(" %llu\n", (unsigned long long)g.tp);
        return 0;
    }
    return 1;
}
