// The per-pair rule and the host-side checks of the spread-limited selection
// (adaptive non-maximal suppression; sift_mi_select_spread_device,
// tests/select_ref.py is the definition).  No HIP runtime in it, so that the
// same text is select.hip's, api.cpp's and a stand-alone program's for the
// sanitizers (tests/host_select_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SIFTMI_SELECT_HD __host__ __device__ __forceinline__
#else
#define SIFTMI_SELECT_HD inline
#endif

namespace siftmi {

constexpr uint32_t kSelectChunk = 1024;  // candidates per LDS stage of k_select_radius (16 B each)
constexpr size_t kSelectMaxRows = 0x7fffffff;

// One separately rounded f32 product / sum.  The squared distance must not be
// fused: a * a + b * b contracted into fma(a, a, b * b) rounds once where the
// rule rounds twice, and the two differ in the last bit often enough to move a
// cut (the restatement's "fused" fixture).
SIFTMI_SELECT_HD float select_mul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    volatile float p = a * b;  // (a rounded f32 the host compiler cannot fold into an fma)
    return p;
#endif
}
SIFTMI_SELECT_HD float select_add(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    volatile float s = a + b;
    return s;
#endif
}

// A candidate j enters the test as c * r_j, computed once.
SIFTMI_SELECT_HD float select_scaled(float c, float r_j) { return select_mul(c, r_j); }
// Row j suppresses row i: strict, so rows of equal response never suppress
// each other and, with 0 < c <= 1 and r >= 0, a row never suppresses itself
// (c * r rounds to at most r).
SIFTMI_SELECT_HD bool select_suppresses(float r_i, float cr_j) { return r_i < cr_j; }
// (x_j - x_i)^2 + (y_j - y_i)^2 in four rounded operations and one rounded sum.
SIFTMI_SELECT_HD float select_dist2(float xi, float yi, float xj, float yj) {
    const float dx = xj - xi, dy = yj - yi;
    return select_add(select_mul(dx, dx), select_mul(dy, dy));
}

// ---- host-side checks: a message for SIFT_MI_EINVAL, or null ---------------------
inline const char* select_params_error(uint32_t limit, float c) {
    if (limit == 0) return "limit must be >= 1";
    if (!(c > 0.0f && c <= 1.0f)) return "c must be in (0, 1]";
    return nullptr;
}
inline const char* select_arena_error(const void* d_kps, const void* d_desc, const size_t* offsets, uint32_t n_segs) {
    if (((uintptr_t)d_kps & 3) != 0) return "d_kps must be 4-byte aligned";
    if (((uintptr_t)d_desc & 15) != 0) return "d_desc must be 16-byte aligned";
    for (uint32_t s = 0; s < n_segs; s++)
        if (offsets[s + 1] < offsets[s]) return "offsets decrease";
    if (offsets[n_segs] - offsets[0] > kSelectMaxRows) return "segments sum to more than 2^31 - 1 rows";
    return nullptr;
}
// sel_offsets[n_segs + 1] of valid offsets: segment s keeps min(n_s, limit) rows.
inline void select_fill_offsets(const size_t* offsets, uint32_t n_segs, uint32_t limit, size_t* sel_offsets) {
    sel_offsets[0] = 0;
    for (uint32_t s = 0; s < n_segs; s++) {
        const size_t n = offsets[s + 1] - offsets[s];
        sel_offsets[s + 1] = sel_offsets[s] + (n < limit ? n : (size_t)limit);
    }
}

}  // namespace siftmi
