// Frame-pair proposal: preemptive matching of each frame's largest-scale
// features (C. Wu, "Towards linear-time incremental structure from motion",
// 3DV 2013).  LABELLED EXTENSION; tests/pairs_ref.py is the definition and
// every output is an integer that equals it.
//
//   k_pairs_select  one workgroup per segment: the h rows with the largest
//                   keypoint size (u32 pattern descending, lower row first
//                   among equals), in ascending row order, gathered into a
//                   compact [n_segs * h] descriptor arena with their row term
//                   m = |x|^2 - 256 sum x (k_match_seg_norms' term);
//   k_pairs_tile    one workgroup per unordered frame pair a < b: with
//                   h <= 128 the 128 x 128 tile of the i8 MFMA matcher is the
//                   whole pair, so top 2 of rows and of columns, both cross
//                   checks, both ratio tests and both counts finish inside the
//                   workgroup and the pair leaves as two integers,
//                   score[a][b] and score[b][a].
//
// Neither kernel touches the segmented matcher's best / second / col_best
// scratch, uses a global atomic or depends on the order of the workgroups.
#include "match_common.h"

namespace siftmi {

// keypoint i's size as its u32 pattern (OutKp: x, y, size, angle, response)
__device__ __forceinline__ uint32_t size_key(const uint32_t* __restrict__ kp_words, uint32_t row) {
    return kp_words[(size_t)row * (sizeof(OutKp) / 4) + 2];
}

// offs[n_segs + 1]: the segments' first rows (relative to kps / d).  Writes
// cnt[s] = min(n_s, h), the selected rows' descriptors sub_d[(s * h + j) * 128]
// and terms sub_m[s * h + j] for j < cnt[s] (the rest of a segment's h slots
// is left as it is and never read), and the score matrix's diagonal.
__global__ __launch_bounds__(256) void k_pairs_select(const uint32_t* __restrict__ kp_words,
                                                      const uint8_t* __restrict__ d,
                                                      const uint32_t* __restrict__ offs, uint32_t n_segs, uint32_t h,
                                                      uint32_t* __restrict__ cnt, uint8_t* __restrict__ sub_d,
                                                      int* __restrict__ sub_m, uint32_t* __restrict__ score) {
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_wsum[4];
    __shared__ uint32_t s_bin, s_above;
    __shared__ uint32_t s_wgt[4], s_weq[4];
    __shared__ uint32_t s_sel[128];
    const uint32_t seg = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t row0 = offs[seg], n = offs[seg + 1] - row0;
    const uint32_t take = min(n, h);
    if (t == 0) {
        cnt[seg] = take;
        score[(size_t)seg * n_segs + seg] = 0;
    }
    if (take == 0) return;
    if (t < 128) s_sel[t] = row0;  // (every slot < take is written below; a row of the segment until then)

    // radix select, most significant byte first: the cut key (the take-th
    // largest) and how many rows equal to it are taken.  `need` of the rows
    // whose key starts with `prefix` are still to be found; at least `need`
    // such rows exist.
    uint32_t prefix = 0, need = take;
    if (n > h) {
        for (int pass = 0; pass < 4; pass++) {
            const int shift = 24 - 8 * pass;
            s_hist[t] = 0;
            __syncthreads();
            for (uint32_t i = t; i < n; i += 256) {
                const uint32_t k = size_key(kp_words, row0 + i);
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
    const bool all = n <= h;
    uint32_t gt_before = 0, eq_before = 0;
    for (uint32_t base = 0; base < n; base += 256) {
        const uint32_t i = base + t;
        bool gt = false, eq = false;
        if (i < n) {
            const uint32_t k = size_key(kp_words, row0 + i);
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
            if (slot < take) s_sel[slot] = row0 + i;  // (always: the guard keeps a mistake inside s_sel)
        }
        __syncthreads();
        if (gt_before + min(eq_before, need) >= take) break;
    }
    // gather: eight lanes a row, 16 bytes each
    const uint32_t part = t & 7;
    for (uint32_t j = t >> 3; j < take; j += 32) {
        const uint4 w = *reinterpret_cast<const uint4*>(d + (size_t)s_sel[j] * kDescSize + 16 * part);
        const size_t o = (size_t)seg * h + j;
        *reinterpret_cast<uint4*>(sub_d + o * kDescSize + 16 * part) = w;
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
        int s2 = 0, s1 = 0;
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int v = (int)((ws[q] >> (8 * b)) & 0xff);
                s2 += v * v;
                s1 += v;
            }
        int m = s2 - 256 * s1;
        m += __shfl_xor(m, 1);
        m += __shfl_xor(m, 2);
        m += __shfl_xor(m, 4);
        if (part == 0) sub_m[o] = m;
    }
}

// In-wave key (d^2 << 6 | index in the wave's 64) -> workgroup key
// (d^2 << 7 | index in the tile's 128); an invalid one -> ~0 (valid d^2 < 2^23)
__device__ __forceinline__ uint32_t tile_key(uint32_t k, uint32_t off) {
    return k >= kBadKey ? ~0u : ((k >> 6) << 7) | (off + (k & 63));
}

// One direction's count: queries i < n whose top 2 over the other side are
// mine[0][i], mine[1][i] (the two waves' halves) and kept by the cross check
// against theirs[.][j].x and the ratio test (match_ref.match, cross_check)
__device__ __forceinline__ uint32_t count_kept(const uint2 (*mine)[128], const uint2 (*theirs)[128], uint32_t n,
                                               uint32_t lane, float ratio) {
    uint32_t kept = 0;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const uint32_t i = lane + 64 * k;
        bool keep = false;
        if (i < n) {
            const uint2 x0 = mine[0][i], x1 = mine[1][i];
            uint32_t lo = x0.x, hi = x0.y;
            merge2(lo, hi, x1.x, x1.y);
            if (lo != ~0u) {
                const uint32_t j = lo & 127;
                keep = (min(theirs[0][j].x, theirs[1][j].x) & 127) == i;
                // batchDistL2_8u32f: sqrt((float) int); no second neighbour: rejected
                if (keep && ratio > 0.0f)
                    keep = hi != ~0u && sqrtf((float)(lo >> 7)) < ratio * sqrtf((float)(hi >> 7));
            }
        }
        kept += (uint32_t)__popcll(__ballot(keep));
    }
    return kept;
}

// Block t is the pair (a, b), a < b, t = b (b - 1) / 2 + a; rows are S_a,
// columns S_b.  The d^2 identity, the fragment layout and the row reduction
// are k_match_seg_tiles' (match.hip), and so is the (256, 3) bound that keeps
// the accumulators in the VGPRs.
__global__ __launch_bounds__(256, 3) void k_pairs_tile(const uint8_t* __restrict__ sub_d, const int* __restrict__ sub_m,
                                                    const uint32_t* __restrict__ cnt, uint32_t n_segs, uint32_t h,
                                                    float ratio, uint32_t* __restrict__ score) {
    uint32_t sb = (uint32_t)((1.0f + sqrtf(1.0f + 8.0f * (float)blockIdx.x)) * 0.5f);
    while (sb * (sb - 1) / 2 > blockIdx.x) sb--;
    while ((sb + 1) * sb / 2 <= blockIdx.x) sb++;
    const uint32_t sa = blockIdx.x - sb * (sb - 1) / 2;
    if (sb >= n_segs) return;  // (never: the grid is n_segs (n_segs - 1) / 2)
    const int nq = (int)cnt[sa], nt = (int)cnt[sb];
    const uint8_t* __restrict__ q = sub_d + (size_t)sa * h * kDescSize;
    const uint8_t* __restrict__ t = sub_d + (size_t)sb * h * kDescSize;
    const int* __restrict__ qn = sub_m + (size_t)sa * h;
    const int* __restrict__ tn = sub_m + (size_t)sb * h;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int q0 = (wave >> 1) * 64;  // this wave's 64 rows
    const int t0 = (wave & 1) * 64;   // and 64 columns
    __shared__ int s_qn[128];
    // top 2 of every row over each column half, of every column over each row half
    __shared__ uint2 s_row[2][128], s_col[2][128];
    if (threadIdx.x < 128) s_qn[threadIdx.x] = (int)threadIdx.x < nq ? qn[threadIdx.x] : kBadD2;
    i32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[a][b][e] = 0;
#pragma unroll
    for (int s = 0; s < kDescSize / 32; s++) {
        const int k0 = 64 * hh + 16 * s;
        i32x4 fa[2], fb[2];
#pragma unroll
        for (int a = 0; a < 2; a++) fa[a] = load_frag_i8(q, q0 + 32 * a + r, nq, k0);
#pragma unroll
        for (int b = 0; b < 2; b++) fb[b] = load_frag_i8(t, t0 + 32 * b + r, nt, k0);
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++)
                acc[a][b] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
    __syncthreads();
    // C/D: column = lane & 31, row = (e & 3) + 8 * (e >> 2) + 4 * hh
    int tnorm[2];
#pragma unroll
    for (int b = 0; b < 2; b++) {
        const int tc = t0 + 32 * b + r;
        tnorm[b] = (tc < nt ? tn[tc] : kBadD2) + (1 << 22);
    }
    uint32_t clo[2] = {~0u, ~0u}, chi[2] = {~0u, ~0u};
    uint32_t rlo[2], rhi[2];
#pragma unroll
    for (int a = 0; a < 2; a++) {
        uint32_t lo[16], hi[16];
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int lr = 32 * a + (e & 3) + 8 * (e >> 2) + 4 * hh;  // row within the wave's 64
            const int qnv = s_qn[q0 + lr];
            uint32_t kr[2];
#pragma unroll
            for (int b = 0; b < 2; b++) {
                const uint32_t di = (uint32_t)(qnv + tnorm[b] - 2 * acc[a][b][e]);  // d^2 (< 2^26 with the bad marks)
                kr[b] = (di << 6) | (uint32_t)(32 * b + r);
                const uint32_t kc = (di << 6) | (uint32_t)lr;
                chi[b] = min(chi[b], max(clo[b], kc));
                clo[b] = min(clo[b], kc);
            }
            lo[e] = min(kr[0], kr[1]);
            hi[e] = max(kr[0], kr[1]);
        }
        fold_rows<16>(lo, hi, 16, (r & 16) != 0);
        fold_rows<8>(lo, hi, 8, (r & 8) != 0);
        fold_rows<4>(lo, hi, 4, (r & 4) != 0);
        fold_rows<2>(lo, hi, 2, (r & 2) != 0);
        rlo[a] = lo[0];
        rhi[a] = hi[0];
    }
    {
        // last step across lane bit 0: even lanes finish tile a = 0, odd lanes a = 1
        const bool up = (r & 1) != 0;
        uint32_t klo = up ? rlo[1] : rlo[0], khi = up ? rhi[1] : rhi[0];
        const uint32_t slo = up ? rlo[0] : rlo[1], shi = up ? rhi[0] : rhi[1];
        merge2(klo, khi, __shfl_xor(slo, 1), __shfl_xor(shi, 1));
        const int e = r >> 1;  // bits 4..1 of the lane chose the row at the four fold steps
        const int lr = 32 * (r & 1) + (e & 3) + 8 * (e >> 2) + 4 * hh;
        s_row[wave & 1][q0 + lr] = make_uint2(tile_key(klo, (uint32_t)t0), tile_key(khi, (uint32_t)t0));
    }
    // the columns' top 2 over both lane halves
#pragma unroll
    for (int b = 0; b < 2; b++) {
        merge2(clo[b], chi[b], __shfl_xor(clo[b], 32), __shfl_xor(chi[b], 32));
        const uint2 top = make_uint2(tile_key(clo[b], (uint32_t)q0), tile_key(chi[b], (uint32_t)q0));
        if (hh == 0) s_col[wave >> 1][t0 + 32 * b + r] = top;
    }
    __syncthreads();
    // wave 0 counts direction a -> b, wave 1 direction b -> a
    if (wave == 0) {
        const uint32_t kept = count_kept(s_row, s_col, (uint32_t)nq, (uint32_t)lane, ratio);
        if (lane == 0) score[(size_t)sa * n_segs + sb] = kept;
    } else if (wave == 1) {
        const uint32_t kept = count_kept(s_col, s_row, (uint32_t)nt, (uint32_t)lane, ratio);
        if (lane == 0) score[(size_t)sb * n_segs + sa] = kept;
    }
}

void launch_pairs(const OutKp* kps, const uint8_t* d, const uint32_t* offs, uint32_t n_segs, uint32_t h, float ratio,
                  uint32_t* cnt, uint8_t* sub_d, int* sub_m, uint32_t* score, hipStream_t st) {
    if (n_segs == 0) return;
    hipLaunchKernelGGL(k_pairs_select, dim3(n_segs), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(kps), d, offs,
                       n_segs, h, cnt, sub_d, sub_m, score);
    const uint32_t tiles = n_segs * (n_segs - 1) / 2;
    if (tiles)
        hipLaunchKernelGGL(k_pairs_tile, dim3(tiles), dim3(256), 0, st, sub_d, sub_m, cnt, n_segs, h, ratio, score);
}

}  // namespace siftmi
