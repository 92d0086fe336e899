// The track builder's union-find (sift-features_amd/csrc/track_common.h) with
// std::atomic, from 8 threads, as a stand-alone program for the sanitizers
// (tests/test_host_tracks.py builds and runs it; nothing is loaded into
// Python).  Input (argv[1]), any number of graphs:
//     graph NAME N E
//     a b            (E lines: rows to join)
// Output per graph: "labels NAME l_0 ... l_{N-1}" (each row's root after all
// unions: the smallest row of its component) and "steps NAME steps retries"
// (walk steps and lost link races, summed over the threads).  The threads
// run in lockstep, one edge each per round, so that links race.
// Every walk and every union is counted against its bound (a walk from x
// takes at most x steps; a union of a, b at most a + b retries): the program
// aborts past either, so the termination argument is exercised here, before
// the same text runs on a GPU.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "track_common.h"

namespace {

struct HostAtomics {
    using cell = std::atomic<uint32_t>;
    static uint32_t load(const cell* p) { return p->load(std::memory_order_relaxed); }
    static bool cas(cell* p, uint32_t& expected, uint32_t desired) {
        std::this_thread::yield();  // widens the window between a find and its CAS: more lost races
        return p->compare_exchange_strong(expected, desired, std::memory_order_relaxed, std::memory_order_relaxed);
    }
};

struct Bounded {
    uint64_t walks = 0, rounds = 0;
    void walk(uint32_t steps, uint32_t start) {
        walks++;
        if (steps > start) {
            std::fprintf(stderr, "walk from %u took %u steps\n", start, steps);
            std::abort();
        }
    }
    void round(uint32_t n, uint32_t a0, uint32_t b0) {
        rounds++;
        if ((uint64_t)n > (uint64_t)a0 + b0) {
            std::fprintf(stderr, "union of %u, %u retried %u times\n", a0, b0, n);
            std::abort();
        }
    }
};

constexpr int kThreads = 8;

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string tag, name;
    size_t n = 0, e = 0;
    while (in >> tag >> name >> n >> e) {
        if (tag != "graph") return 3;
        std::vector<std::pair<uint32_t, uint32_t>> edges(e);
        for (auto& ed : edges) {
            if (!(in >> ed.first >> ed.second) || ed.first >= n || ed.second >= n) return 4;
        }
        std::unique_ptr<std::atomic<uint32_t>[]> parent(new std::atomic<uint32_t>[n ? n : 1]);
        for (size_t r = 0; r < n; r++) parent[r].store((uint32_t)r, std::memory_order_relaxed);
        Bounded counts[kThreads];
        std::vector<std::thread> pool;
        // Lockstep, as the lanes of a wave: round k hands edges k * 8 .. k * 8 + 7
        // to the 8 threads and releases them together (a counting barrier;
        // host-side only), so neighbouring matches race for the same root.
        std::atomic<size_t> arrived{0};
        const size_t n_rounds = (edges.size() + kThreads - 1) / kThreads;
        for (int t = 0; t < kThreads; t++)
            pool.emplace_back([&, t] {
                for (size_t k = 0; k < n_rounds; k++) {
                    arrived.fetch_add(1);
                    while (arrived.load() < (k + 1) * kThreads) std::this_thread::yield();
                    const size_t i = k * kThreads + t;
                    if (i < edges.size())
                        siftmi::track_union<HostAtomics>(parent.get(), edges[i].first, edges[i].second, counts[t]);
                }
            });
        for (auto& th : pool) th.join();
        // the invariant: parent[x] <= x
        for (size_t r = 0; r < n; r++)
            if (parent[r].load() > r) return 5;
        Bounded flat;
        std::cout << "labels " << name;
        for (size_t r = 0; r < n; r++)
            std::cout << ' ' << siftmi::track_find<HostAtomics>(parent.get(), (uint32_t)r, flat);
        uint64_t walks = flat.walks, rounds = 0;
        for (const Bounded& c : counts) {
            walks += c.walks;
            rounds += c.rounds;
        }
        std::cout << "\nsteps " << name << ' ' << walks << ' ' << rounds << '\n';
    }
    return 0;
}
