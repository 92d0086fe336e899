// The per-pair rule and the host-side checks of the spread-limited selection
// (sift-features_amd/csrc/select_rule.h, the header select.hip includes) as a
// stand-alone program for the sanitizers (tests/test_host_select.py builds
// and runs it; nothing is loaded into Python).  Input (argv[1]), any number of
// cases, every f32 as its u32 pattern:
//     case NAME N_SEGS LIMIT C TOTAL
//     offsets (N_SEGS + 1)
//     x y response (TOTAL rows of three)
// Output per case: "error NAME message" when a check refuses it, else
//     sel NAME sel_offsets...      rows NAME rows...      r2 NAME patterns...
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "select_rule.h"

static float as_float(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static uint32_t as_bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string tag, name;
    uint32_t n_segs, limit, c_bits;
    size_t total;
    while (in >> tag >> name >> n_segs >> limit >> c_bits >> total) {
        if (tag != "case") return 2;
        // exactly as many entries as stated, on the heap: a read past either is the sanitizer's
        std::vector<size_t> offs((size_t)n_segs + 1), sel((size_t)n_segs + 1);
        for (size_t& v : offs)
            if (!(in >> v)) return 2;
        std::vector<float> x(total), y(total), r(total);
        for (size_t i = 0; i < total; i++) {
            uint32_t a, b, c;
            if (!(in >> a >> b >> c)) return 2;
            x[i] = as_float(a), y[i] = as_float(b), r[i] = as_float(c);
        }
        const float c = as_float(c_bits);
        const char* msg = siftmi::select_params_error(limit, c);
        if (!msg) msg = siftmi::select_arena_error(x.data(), nullptr, offs.data(), n_segs);
        if (!msg && offs[n_segs] > total) msg = "offsets reach beyond the rows";
        if (msg) {
            std::cout << "error " << name << ' ' << msg << '\n';
            continue;
        }
        siftmi::select_fill_offsets(offs.data(), n_segs, limit, sel.data());
        std::vector<uint32_t> r2(offs[n_segs] - offs[0]), rows;
        for (uint32_t s = 0; s < n_segs; s++) {
            const size_t lo = offs[s], hi = offs[s + 1];
            std::vector<float> scaled(hi - lo);
            for (size_t j = lo; j < hi; j++) scaled[j - lo] = siftmi::select_scaled(c, r[j]);
            for (size_t i = lo; i < hi; i++) {
                float m = std::numeric_limits<float>::infinity();
                for (size_t j = lo; j < hi; j++)
                    if (siftmi::select_suppresses(r[i], scaled[j - lo]))
                        m = std::min(m, siftmi::select_dist2(x[i], y[i], x[j], y[j]));
                r2[i - offs[0]] = as_bits(m);
            }
            std::vector<uint32_t> order(hi - lo);
            for (size_t i = 0; i < order.size(); i++) order[i] = (uint32_t)i;
            const uint32_t* key = r2.data() + (lo - offs[0]);
            std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] > key[b]; });
            order.resize(sel[s + 1] - sel[s]);
            std::sort(order.begin(), order.end());
            rows.insert(rows.end(), order.begin(), order.end());
        }
        std::cout << "sel " << name;
        for (size_t v : sel) std::cout << ' ' << v;
        std::cout << "\nrows " << name;
        for (uint32_t v : rows) std::cout << ' ' << v;
        std::cout << "\nr2 " << name;
        for (uint32_t v : r2) std::cout << ' ' << v;
        std::cout << '\n';
    }
    return 0;
}
