// Baseline of tools/bench_tracks.py: a plain single-thread union-find (path
// halving, smaller root wins) over an edge list.  argv[1]: a binary file of
// uint32 -- N, E, then E pairs of rows.  Prints "components ms", the time of
// the unions plus the final labelling, without the file read.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t head[2];
    if (std::fread(head, 4, 2, f) != 2) return 4;
    const uint32_t n = head[0], e = head[1];
    std::vector<uint32_t> ed(2 * (size_t)e);
    if (e && std::fread(ed.data(), 8, e, f) != e) return 4;
    std::fclose(f);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> parent(n), label(n);
    for (uint32_t r = 0; r < n; r++) parent[r] = r;
    auto find = [&](uint32_t x) {
        while (parent[x] != x) {
            parent[x] = parent[parent[x]];
            x = parent[x];
        }
        return x;
    };
    for (uint32_t i = 0; i < e; i++) {
        if (ed[2 * i] >= n || ed[2 * i + 1] >= n) return 5;
        const uint32_t a = find(ed[2 * i]), b = find(ed[2 * i + 1]);
        if (a != b) parent[a > b ? a : b] = a > b ? b : a;
    }
    size_t comps = 0;
    for (uint32_t r = 0; r < n; r++) comps += (label[r] = find(r)) == r;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::printf("%zu %.3f\n", comps, ms);
    return 0;
}
