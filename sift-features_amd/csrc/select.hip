// Spread-limited keypoints: adaptive non-maximal suppression (Brown, Szeliski,
// Winder, "Multi-image matching using multi-scale oriented patches", CVPR
// 2005).  LABELLED EXTENSION; tests/select_ref.py is the definition and every
// output equals it bit for bit.
//
//   k_select_radius  one workgroup per (segment, 512 query rows): each lane
//                    holds kSelectQ query rows in registers; the segment's
//                    candidates (x, y, c * r) pass through LDS kSelectChunk at
//                    a time, 16 B each, every lane reading the same address (one
//                    broadcast LDS read a candidate).  R2 = the least unfused squared
//                    distance to a candidate with r_i < c * r_j, +inf without
//                    one.  A minimum: no order of lanes or chunks can show.
//   k_select_pick    one workgroup per segment: the min(n, limit) rows with the
//                    largest R2 pattern (lower row first among equals) by a
//                    radix select, emitted in ascending row order
//                    (k_pairs_select's rule and form).
//   k_select_gather  eight lanes a kept row: its keypoint and, when there are
//                    descriptors, its 128 bytes in 16-byte moves into the
//                    compact arena.
//
// No global atomic; a lane only ever reads rows of its own segment.
#include "select_rule.h"
#include "sift_common.h"
#include "sift_kernels.h"

namespace siftmi {

constexpr int kSelectQ = 2;  // query rows per lane
constexpr uint32_t kSelectThreads = 256;
static_assert(kSelectRowsPerWg == kSelectThreads * kSelectQ, "sift_kernels.h states the rows of a workgroup");
static_assert(kSelectChunk % kSelectThreads == 0 && kSelectChunk % 4 == 0, "staging and the unrolled walk");
constexpr int kKpWords = sizeof(OutKp) / 4;  // x, y, size, angle, response
constexpr uint32_t kInfBits = 0x7f800000u;

// wgs[b] = (segment, first query row of workgroup b within it); offs[n_segs +
// 1]: the segments' first rows from kp on.  r2[row] for every row of every
// segment.
__global__ __launch_bounds__(kSelectThreads) void k_select_radius(const float* __restrict__ kp,
                                                                  const uint32_t* __restrict__ offs,
                                                                  const uint2* __restrict__ wgs, float c,
                                                                  float* __restrict__ r2) {
    __shared__ float4 s_cand[kSelectChunk];
    const uint2 wg = wgs[blockIdx.x];
    const uint32_t t = threadIdx.x;
    const uint32_t row0 = offs[wg.x], n = offs[wg.x + 1] - row0;
    const float inf = __builtin_inff();
    float qx[kSelectQ], qy[kSelectQ], qr[kSelectQ];
    uint32_t m[kSelectQ];  // R2 as its pattern
#pragma unroll
    for (int q = 0; q < kSelectQ; q++) {
        const uint32_t i = wg.y + (uint32_t)q * kSelectThreads + t;
        qx[q] = qy[q] = 0.0f;
        qr[q] = inf;  // a lane past the segment's end: nothing suppresses it, nothing is stored
        if (i < n) {
            const float* p = kp + (size_t)(row0 + i) * kKpWords;
            qx[q] = p[0];
            qy[q] = p[1];
            qr[q] = p[4];
        }
        m[q] = kInfBits;
    }
    for (uint32_t base = 0; base < n; base += kSelectChunk) {
        const uint32_t cnt = min(kSelectChunk, n - base);
        __syncthreads();  // the walk over the previous chunk is over
#pragma unroll
        for (uint32_t k = t; k < kSelectChunk; k += kSelectThreads) {
            float4 v = make_float4(0.0f, 0.0f, -inf, 0.0f);  // past the chunk's rows: suppresses nothing
            if (k < cnt) {
                const float* p = kp + (size_t)(row0 + base + k) * kKpWords;
                v = make_float4(p[0], p[1], select_scaled(c, p[4]), 0.0f);
            }
            s_cand[k] = v;
        }
        __syncthreads();
        const uint32_t lim = (cnt + 3u) & ~3u;
#pragma unroll 4
        for (uint32_t k = 0; k < lim; k++) {
            const float4 v = s_cand[k];
#pragma unroll
            for (int q = 0; q < kSelectQ; q++) {
                // d is +0 or above, or a NaN: on the u32 patterns the minimum is the
                // numeric one, and a NaN of either sign lies above +inf and never wins
                const uint32_t d = __float_as_uint(select_dist2(qx[q], qy[q], v.x, v.y));
                m[q] = min(m[q], select_suppresses(qr[q], v.z) ? d : kInfBits);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < kSelectQ; q++) {
        const uint32_t i = wg.y + (uint32_t)q * kSelectThreads + t;
        if (i < n) r2[row0 + i] = __uint_as_float(m[q]);
    }
}

// sel_offs[n_segs + 1]: the segments' first kept rows (sel_offs[s + 1] -
// sel_offs[s] = min(n_s, limit), the host's sums).  rows[o] = the kept row
// within its segment, src[o] = the same from the arena's first row on.
__global__ __launch_bounds__(256) void k_select_pick(const uint32_t* __restrict__ r2_words,
                                                     const uint32_t* __restrict__ offs,
                                                     const uint32_t* __restrict__ sel_offs, uint32_t limit,
                                                     uint32_t* __restrict__ rows, uint32_t* __restrict__ src) {
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_wsum[4];
    __shared__ uint32_t s_bin, s_above;
    __shared__ uint32_t s_wgt[4], s_weq[4];
    const uint32_t seg = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t row0 = offs[seg], n = offs[seg + 1] - row0;
    const uint32_t take = min(n, limit), out0 = sel_offs[seg];
    if (take == 0) return;
    const uint32_t* __restrict__ key = r2_words + row0;

    // radix select, most significant byte first: the cut key (the take-th
    // largest) and how many rows equal to it are taken.  `need` of the rows
    // whose key starts with `prefix` are still to be found; at least `need`
    // such rows exist.
    const bool all = n <= limit;
    uint32_t prefix = 0, need = take;
    if (!all) {
        for (int pass = 0; pass < 4; pass++) {
            const int shift = 24 - 8 * pass;
            s_hist[t] = 0;
            __syncthreads();
            for (uint32_t i = t; i < n; i += 256) {
                const uint32_t k = key[i];
                if (pass == 0 || (k >> (shift + 8)) == prefix) atomicAdd(&s_hist[(k >> shift) & 255], 1u);
            }
            __syncthreads();
            // ge = rows in bins >= t: a suffix sum over the wave, then over the waves
            const uint32_t own = s_hist[t];
            uint32_t ge = own;
#pragma unroll
            for (int dd = 1; dd < 64; dd <<= 1) {
                const uint32_t o = __shfl_down(ge, dd);
                if (lane + dd < 64) ge += o;
            }
            if (lane == 0) s_wsum[wave] = ge;
            __syncthreads();
            for (uint32_t w = wave + 1; w < 4; w++) ge += s_wsum[w];
            const uint32_t above = ge - own;
            if (above < need && need <= ge) {  // exactly one bin
                s_bin = t;
                s_above = above;
            }
            __syncthreads();
            prefix = (prefix << 8) | s_bin;
            need -= s_above;
        }
    }
    // emission in ascending row order: a row is taken when its key is above
    // the cut, or equals it and fewer than `need` equal rows precede it; its
    // slot is the number of taken rows before it (an ordered prefix over the
    // segment, 256 rows a step)
    uint32_t gt_before = 0, eq_before = 0;
    for (uint32_t base = 0; base < n; base += 256) {
        const uint32_t i = base + t;
        bool gt = false, eq = false;
        if (i < n) {
            const uint32_t k = key[i];
            gt = all || k > prefix;
            eq = !all && k == prefix;
        }
        const unsigned long long mg = __ballot(gt), me = __ballot(eq);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (lane == 0) {
            s_wgt[wave] = (uint32_t)__popcll(mg);
            s_weq[wave] = (uint32_t)__popcll(me);
        }
        __syncthreads();
        uint32_t g = gt_before + (uint32_t)__popcll(mg & below), e = eq_before + (uint32_t)__popcll(me & below);
        for (uint32_t w = 0; w < 4; w++) {
            if (w < wave) {
                g += s_wgt[w];
                e += s_weq[w];
            }
            gt_before += s_wgt[w];
            eq_before += s_weq[w];
        }
        if (gt || (eq && e < need)) {
            const uint32_t slot = g + min(e, need);
            if (slot < take) {  // (always: the guard keeps a mistake inside the segment's range)
                rows[out0 + slot] = i;
                src[out0 + slot] = row0 + i;
            }
        }
        __syncthreads();
        if (gt_before + min(eq_before, need) >= take) break;
    }
}

// Kept row o of `total`: eight lanes, five of them a keypoint word each, all
// of them 16 descriptor bytes each when d is not null.
__global__ __launch_bounds__(256) void k_select_gather(const uint32_t* __restrict__ kp_words,
                                                       const uint8_t* __restrict__ d,
                                                       const uint32_t* __restrict__ src, uint32_t total,
                                                       uint32_t n_rows,
                                                       uint32_t* __restrict__ out_kp_words,
                                                       uint8_t* __restrict__ out_d) {
    const uint32_t o = blockIdx.x * 32 + (threadIdx.x >> 3), part = threadIdx.x & 7;
    if (o >= total) return;
    const uint32_t r = src[o];
    if (r >= n_rows) return;  // (never: k_select_pick fills every slot with a row of the arena)
    if (part < kKpWords) out_kp_words[(size_t)o * kKpWords + part] = kp_words[(size_t)r * kKpWords + part];
    if (d)
        *reinterpret_cast<uint4*>(out_d + (size_t)o * kDescSize + 16 * part) =
            *reinterpret_cast<const uint4*>(d + (size_t)r * kDescSize + 16 * part);
}

void launch_select(const SelectLaunch& L, hipStream_t st) {
    if (L.n_wgs)
        hipLaunchKernelGGL(k_select_radius, dim3(L.n_wgs), dim3(kSelectThreads), 0, st,
                           reinterpret_cast<const float*>(L.kps), L.offs, L.wgs, L.c, L.r2);
    if (L.n_segs && L.total)
        hipLaunchKernelGGL(k_select_pick, dim3(L.n_segs), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(L.r2),
                           L.offs, L.sel_offs, L.limit, L.rows, L.src);
    if (L.total)
        hipLaunchKernelGGL(k_select_gather, dim3((L.total + 31) / 32), dim3(256), 0, st,
                           reinterpret_cast<const uint32_t*>(L.kps), L.d, L.src, L.total, L.n_rows,
                           reinterpret_cast<uint32_t*>(L.sel_kps), L.sel_d);
}

}  // namespace siftmi
