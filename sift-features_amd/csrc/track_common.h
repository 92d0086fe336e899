// Lock-free union-find of the track builder (tracks.hip), as functions
// templated on the atomic primitives: the same text is the link kernel's body
// on the device (agent-scope relaxed atomics) and, with std::atomic, the body
// of a host program that runs it from several threads under the sanitizers
// (tests/host_tracks_main.cpp).
//
// INVARIANT, at every instant: parent[x] <= x, and parent[x] is x itself (x
// is a root) or an ancestor of x.  The only writes are
//   link      CAS parent[r]: r -> s, with s < r a node of another tree
//             (expected value r: only a root is ever linked, and only once);
//   halving   CAS parent[x]: p -> parent[p], with p = parent[x] != x (never a
//             root's cell, and the new value is an ancestor smaller than p).
// Both keep the invariant, so
//   * every walk x -> parent[x] -> ... strictly decreases and ends at a root
//     after at most x steps, on stale values too: a stale parent is still an
//     ancestor;
//   * a link's CAS fails only if its cell stopped being a root, which only
//     another successful link does; the loser resumes from the value read
//     back, which is smaller: its (a + b) strictly decreases per round, and
//     there are at most N - 1 successful links in all.
// No loop here waits for another thread: there is no lock, flag or spin.
//
// A supplies   cell                          the array's element type
//              load(const cell*)             relaxed atomic load
//              cas(cell*, uint32_t& expected, uint32_t desired)
//                                            relaxed strong CAS; on failure
//                                            `expected` holds the value read
// C counts     walk(uint32_t steps, uint32_t start), round(rounds, a0, b0)
//              (the host program aborts past the bounds above; the device
//              passes TrackNoCount).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TRACK_FN __device__ __forceinline__
#else
#define TRACK_FN inline
#endif

namespace siftmi {

struct TrackNoCount {
    TRACK_FN void walk(uint32_t, uint32_t) {}
    TRACK_FN void round(uint32_t, uint32_t, uint32_t) {}
};

// Root of x's tree as of some instant during the call, halving the path on
// the way.  At most x steps.
template <class A, class C>
TRACK_FN uint32_t track_find(typename A::cell* parent, uint32_t x, C& count) {
    const uint32_t start = x;
    uint32_t steps = 0;
    for (;;) {
        const uint32_t p = A::load(parent + x);
        if (p == x) return x;
        const uint32_t g = A::load(parent + p);  // g <= p < x
        if (g != p) {
            uint32_t expected = p;
            (void)A::cas(parent + x, expected, g);  // a lost race leaves another ancestor there
        }
        x = p;
        count.walk(++steps, start);
    }
}

// Joins the trees of a and b: the larger root goes under the smaller.
template <class A, class C>
TRACK_FN void track_union(typename A::cell* parent, uint32_t a, uint32_t b, C& count) {
    const uint32_t a0 = a, b0 = b;
    uint32_t rounds = 0;
    for (;;) {
        a = track_find<A>(parent, a, count);
        b = track_find<A>(parent, b, count);
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        uint32_t expected = a;
        if (A::cas(parent + a, expected, b)) return;
        a = expected;  // < the old a: someone else linked it first
        count.round(++rounds, a0, b0);
    }
}

}  // namespace siftmi
