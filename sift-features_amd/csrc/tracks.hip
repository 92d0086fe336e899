// Feature tracks on MI355X: the connected components of the graph whose nodes
// are the arena's keypoint rows and whose edges are the kept matches
// (LABELLED EXTENSION; tests/tracks_ref.py is the definition).
//
//   k_track_init     parent[r] = r, seg_of[r] (search over the offsets in LDS)
//   k_track_link     one lane per match: lock-free union (track_common.h)
//   k_track_flatten  label[r] = root(r): the component's smallest row
//   radix sort       rocPRIM, stable, (label, row) with rows fed ascending:
//                    members by (label, row)
//   k_track_runs     per component: first / last sorted position, conflict
//   k_track_count    per 256 sorted positions: kept tracks, kept members
//   k_track_scan     one workgroup: exclusive scan of those block counts
//   k_track_emit     track_of, track_offsets, conflict, obs (gathered from the
//                    keypoints); positions from wave ballots + the block scan,
//                    so they do not depend on arrival order
//
// Every loop's bound: the walks of k_track_link / k_track_flatten strictly
// decrease (track_common.h, at most r steps from row r; a link retries at
// most a + b times); the binary searches halve a range of n_segs / n_pairs
// entries; k_track_scan runs ceil(n_blocks / 256) rounds; the
// LDS fills are strided copies.  Nothing waits for another lane.
//
// Coherence: within k_track_link every access to parent[] is an agent-scope
// relaxed atomic (the XCDs' L2s are not coherent for plain accesses within a
// launch).  Every other kernel reads what an earlier launch wrote.
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstddef>

#include "sift_common.h"
#include "sift_kernels.h"
#include "track_common.h"

namespace siftmi {

namespace {

constexpr int kTrackBlock = 256;

struct DeviceAtomics {
    using cell = uint32_t;
    static __device__ __forceinline__ uint32_t load(const uint32_t* p) {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ bool cas(uint32_t* p, uint32_t& expected, uint32_t desired) {
        return __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
    }
};

// Largest i in [0, n) with tab[i * kStride] <= v; tab[0] <= v is the caller's
// promise (equal entries, i.e. empty segments / pairs: the last of them).
template <int kStride>
__device__ __forceinline__ uint32_t last_not_above(const uint32_t* tab, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {  // hi - lo halves
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (tab[(size_t)mid * kStride] <= v)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kTrackBlock) void k_track_init(const uint32_t* __restrict__ offs, uint32_t n_segs,
                                                            uint32_t n, uint32_t* __restrict__ parent,
                                                            uint32_t* __restrict__ seg_of,
                                                            uint8_t* __restrict__ confl) {
    __shared__ uint32_t s_off[kTrackLdsSegs];
    const bool lds = n_segs <= kTrackLdsSegs;
    if (lds) {
        for (uint32_t i = threadIdx.x; i < n_segs; i += kTrackBlock) s_off[i] = offs[i];
        __syncthreads();
    }
    const uint32_t r = blockIdx.x * kTrackBlock + threadIdx.x;
    if (r >= n) return;
    parent[r] = r;
    confl[r] = 0;
    seg_of[r] = lds ? last_not_above<1>(s_off, n_segs, r) : last_not_above<1>(offs, n_segs, r);
}

static_assert(sizeof(TrackPair) == 3 * sizeof(uint32_t) && offsetof(TrackPair, rec0) == 0,
              "the pair search strides over rec0");

__global__ __launch_bounds__(kTrackBlock) void k_track_link(const VerifyMatch* __restrict__ matches,
                                                            const uint8_t* __restrict__ keep,
                                                            const TrackPair* __restrict__ pairs, uint32_t n_pairs,
                                                            uint32_t n_matches, uint32_t* parent) {
    const uint32_t m = blockIdx.x * kTrackBlock + threadIdx.x;
    if (m >= n_matches) return;
    if (keep && !keep[m]) return;
    const TrackPair pr = pairs[last_not_above<3>(&pairs->rec0, n_pairs, m)];
    const uint32_t a = pr.qrow0 + (uint32_t)matches[m].query_idx, b = pr.trow0 + (uint32_t)matches[m].train_idx;
    TrackNoCount none;
    track_union<DeviceAtomics>(parent, a, b, none);
}

// After every link: plain reads of parent[] (an earlier launch wrote it).
__global__ __launch_bounds__(kTrackBlock) void k_track_flatten(const uint32_t* __restrict__ parent, uint32_t n,
                                                               uint32_t* __restrict__ label,
                                                               uint32_t* __restrict__ row) {
    const uint32_t r = blockIdx.x * kTrackBlock + threadIdx.x;
    if (r >= n) return;
    uint32_t x = r;
    for (uint32_t p = parent[x]; p != x; p = parent[x]) x = p;  // p < x: at most r steps
    label[r] = x;
    row[r] = r;
}

// sl / sr: the sorted labels and rows.  Position i is the first of its
// component iff i == start[label], and the component is [start, end).
__global__ __launch_bounds__(kTrackBlock) void k_track_runs(const uint32_t* __restrict__ sl,
                                                            const uint32_t* __restrict__ sr,
                                                            const uint32_t* __restrict__ seg_of, uint32_t n,
                                                            uint32_t* __restrict__ start, uint32_t* __restrict__ end,
                                                            uint8_t* __restrict__ confl) {
    const uint32_t i = blockIdx.x * kTrackBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t l = sl[i];
    const bool head = i == 0 || sl[i - 1] != l;
    if (head) start[l] = i;
    if (i == n - 1 || sl[i + 1] != l) end[l] = i + 1;
    // rows ascend within a component and segments are contiguous: two rows of
    // one segment are adjacent (every writer stores the same 1)
    if (!head && seg_of[sr[i]] == seg_of[sr[i - 1]]) confl[l] = 1;
}

struct TrackFlags {
    bool head, kept;
};
__device__ __forceinline__ TrackFlags track_flags(uint32_t l, uint32_t i, const uint32_t* __restrict__ start,
                                                  const uint32_t* __restrict__ end, const uint8_t* __restrict__ confl,
                                                  uint32_t min_length, int drop) {
    const uint32_t s = start[l];
    TrackFlags f;
    f.head = s == i;
    f.kept = end[l] - s >= min_length && !(drop && confl[l]);
    return f;
}

// Exclusive prefix counts of two flags over the workgroup, and its totals.
__device__ __forceinline__ void block_prefix(bool fa, bool fb, uint32_t& pa, uint32_t& pb, uint32_t& ta,
                                             uint32_t& tb) {
    __shared__ uint32_t s_w[2][kTrackBlock / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long ba = __ballot(fa), bb = __ballot(fb), below = (1ull << lane) - 1;
    if (lane == 0) {
        s_w[0][wv] = __popcll(ba);
        s_w[1][wv] = __popcll(bb);
    }
    __syncthreads();
    pa = __popcll(ba & below);
    pb = __popcll(bb & below);
    ta = tb = 0;
#pragma unroll
    for (int w = 0; w < kTrackBlock / 64; w++) {
        if (w < wv) {
            pa += s_w[0][w];
            pb += s_w[1][w];
        }
        ta += s_w[0][w];
        tb += s_w[1][w];
    }
}

__global__ __launch_bounds__(kTrackBlock) void k_track_count(const uint32_t* __restrict__ sl, uint32_t n,
                                                             const uint32_t* __restrict__ start,
                                                             const uint32_t* __restrict__ end,
                                                             const uint8_t* __restrict__ confl, uint32_t min_length,
                                                             int drop, uint2* __restrict__ bsum) {
    const uint32_t i = blockIdx.x * kTrackBlock + threadIdx.x;
    TrackFlags f{false, false};
    if (i < n) f = track_flags(sl[i], i, start, end, confl, min_length, drop);
    uint32_t pa, pb, ta, tb;
    block_prefix(f.head && f.kept, f.kept, pa, pb, ta, tb);
    if (threadIdx.x == 0) bsum[blockIdx.x] = make_uint2(ta, tb);
}

// One workgroup: bsum[b] becomes the sum of the blocks before b; totals =
// (tracks, members), and the closing entry of track_offsets.
__global__ __launch_bounds__(kTrackBlock) void k_track_scan(uint2* __restrict__ bsum, uint32_t n_blocks,
                                                            uint32_t* __restrict__ totals,
                                                            uint32_t* __restrict__ track_offsets) {
    __shared__ uint2 s_w[kTrackBlock / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint2 carry = make_uint2(0, 0);
    for (uint32_t base = 0; base < n_blocks; base += kTrackBlock) {  // ceil(n_blocks / 256) rounds
        const uint32_t b = base + threadIdx.x;
        const uint2 v = b < n_blocks ? bsum[b] : make_uint2(0, 0);
        uint2 inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t x = __shfl_up(inc.x, o), y = __shfl_up(inc.y, o);
            if (lane >= o) {
                inc.x += x;
                inc.y += y;
            }
        }
        if (lane == 63) s_w[wv] = inc;
        __syncthreads();
        uint2 tot = make_uint2(0, 0);
#pragma unroll
        for (int w = 0; w < kTrackBlock / 64; w++) {
            if (w < wv) {
                inc.x += s_w[w].x;
                inc.y += s_w[w].y;
            }
            tot.x += s_w[w].x;
            tot.y += s_w[w].y;
        }
        if (b < n_blocks) bsum[b] = make_uint2(carry.x + inc.x - v.x, carry.y + inc.y - v.y);
        carry.x += tot.x;
        carry.y += tot.y;
        __syncthreads();  // s_w is rewritten by the next round
    }
    if (threadIdx.x == 0) {
        totals[0] = carry.x;
        totals[1] = carry.y;
        track_offsets[carry.x] = carry.y;
    }
}

__global__ __launch_bounds__(kTrackBlock) void k_track_emit(
    const uint32_t* __restrict__ sl, const uint32_t* __restrict__ sr, uint32_t n, const uint32_t* __restrict__ start,
    const uint32_t* __restrict__ end, const uint8_t* __restrict__ confl, uint32_t min_length, int drop,
    const uint2* __restrict__ bsum, const uint32_t* __restrict__ seg_of, const uint32_t* __restrict__ offs,
    const OutKp* __restrict__ kps, int32_t* __restrict__ track_of, uint32_t* __restrict__ track_offsets,
    TrackObs* __restrict__ obs, uint8_t* __restrict__ conflict) {
    const uint32_t i = blockIdx.x * kTrackBlock + threadIdx.x;
    TrackFlags f{false, false};
    uint32_t l = 0;
    if (i < n) {
        l = sl[i];
        f = track_flags(l, i, start, end, confl, min_length, drop);
    }
    const bool head = f.head && f.kept;
    uint32_t pt, pm, tt, tm;
    block_prefix(head, f.kept, pt, pm, tt, tm);
    if (i >= n) return;
    const uint32_t r = sr[i];
    if (!f.kept) {
        track_of[r] = -1;
        return;
    }
    const uint2 before = bsum[blockIdx.x];
    // kept heads at positions <= i, minus one: a member follows its head
    const uint32_t t = before.x + pt + (head ? 1u : 0u) - 1u, o = before.y + pm;
    track_of[r] = (int32_t)t;
    const uint32_t s = seg_of[r];
    const OutKp k = kps[r];
    TrackObs ob;
    ob.seg = s;
    ob.idx = r - offs[s];
    ob.x = k.x;
    ob.y = k.y;
    obs[o] = ob;
    if (head) {
        track_offsets[t] = o;
        conflict[t] = confl[l];
    }
}

inline unsigned blocks_of(uint32_t n) { return (n + kTrackBlock - 1) / kTrackBlock; }

inline unsigned label_bits(uint32_t n) {
    unsigned bits = 1;
    while (bits < 32 && (1ull << bits) < n) bits++;
    return bits;
}

}  // namespace

size_t track_sort_temp_bytes(uint32_t n) {
    size_t bytes = 0;
    const uint32_t* k = nullptr;
    uint32_t* o = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, bytes, k, o, k, o, n, 0u, label_bits(n), hipStream_t{}) != hipSuccess)
        return 0;
    return std::max<size_t>(bytes, 1);
}

int launch_tracks(const TrackLaunch& L, hipStream_t st) {
    const uint32_t n = L.n_rows;
    if (!n) return 0;
    hipLaunchKernelGGL(k_track_init, dim3(blocks_of(n)), dim3(kTrackBlock), 0, st, L.offs, L.n_segs, n, L.parent,
                       L.seg_of, L.confl);
    if (L.n_matches)
        hipLaunchKernelGGL(k_track_link, dim3(blocks_of(L.n_matches)), dim3(kTrackBlock), 0, st, L.matches, L.keep,
                           L.pairs, L.n_pairs, L.n_matches, L.parent);
    hipLaunchKernelGGL(k_track_flatten, dim3(blocks_of(n)), dim3(kTrackBlock), 0, st, L.parent, n, L.label, L.row);
    size_t bytes = L.sort_temp_bytes;
    if (rocprim::radix_sort_pairs(L.sort_temp, bytes, (const uint32_t*)L.label, L.sorted_label,
                                  (const uint32_t*)L.row, L.sorted_row, n, 0u, label_bits(n), st) != hipSuccess)
        return -1;
    hipLaunchKernelGGL(k_track_runs, dim3(blocks_of(n)), dim3(kTrackBlock), 0, st, L.sorted_label, L.sorted_row,
                       L.seg_of, n, L.start, L.end, L.confl);
    hipLaunchKernelGGL(k_track_count, dim3(blocks_of(n)), dim3(kTrackBlock), 0, st, L.sorted_label, n, L.start, L.end,
                       L.confl, L.min_length, L.drop_conflicts, L.bsum);
    hipLaunchKernelGGL(k_track_scan, dim3(1), dim3(kTrackBlock), 0, st, L.bsum, blocks_of(n), L.totals,
                       L.track_offsets);
    hipLaunchKernelGGL(k_track_emit, dim3(blocks_of(n)), dim3(kTrackBlock), 0, st, L.sorted_label, L.sorted_row, n,
                       L.start, L.end, L.confl, L.min_length, L.drop_conflicts, L.bsum, L.seg_of, L.offs, L.kps,
                       L.track_of, L.track_offsets, L.obs, L.conflict);
    return 0;
}

}  // namespace siftmi
