// Detection-stage micro-benchmarks (performance experiments only; not part of
// libsift_mi.so): blur 4 / blur 5 strips, k_detect_rows, k_blur_detect and
// k_refine on octave 0 of N 1080p frames (3840x2160 seed planes) of smooth
// synthetic content, each launch timed alone with HIP events.  Build:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-honor-nans \
//         tools/ubench_detect.hip -o tools/ubench_detect
// (the scan kernels' flags; the refine kernels here do not depend on NaN
// semantics for the timing A/B)
#include "../sift-features_amd/csrc/detect.hip"
#include "../sift-features_amd/csrc/scan.hip"
#include "../sift-features_amd/csrc/pyramid.hip"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace siftmi;

// the round-4 k_refine (single-float DoG reads), for A/B
namespace siftmi {
struct DogViewOld {
    const gfloat* g;  // G_0 of one frame's octave
    size_t P;         // floats per plane
    __device__ __forceinline__ float operator()(int s, size_t off) const {
        return g[(size_t)(s + 1) * P + off] - g[(size_t)s * P + off];
    }
};

__device__ __forceinline__ bool interpolate_old(const DogViewOld& dv, int W, int H, int pitch, int& scale, int& x, int& y,
                                            float& os, float& ox, float& oy, uint32_t* band_flag, int vlo, int vhi) {
    for (int it = 0; it < kMaxInterpSteps; it++) {
        // row bands with a restricted pyramid (pipeline.cpp PyramidRun): the
        // rows read here must be computed ones, else the host recomputes the
        // band on the whole-frame pyramid
        if (band_flag && (y - 1 < vlo || y + 1 >= vhi)) atomicOr(band_flag, 1u);
        const int prev = scale - 1, curr = scale, next = scale + 1;
#define AT(a, yy, xx) dv(a, (size_t)(yy) * pitch + (xx))
        const float g1 = (AT(next, y, x) - AT(prev, y, x)) / 2.f;
        const float g2 = (AT(curr, y + 1, x) - AT(curr, y - 1, x)) / 2.f;
        const float g3 = (AT(curr, y, x + 1) - AT(curr, y, x - 1)) / 2.f;
        const float v2 = AT(curr, y, x) * 2.f;
        const float h11 = AT(next, y, x) + AT(prev, y, x) - v2;
        const float h12 = (AT(next, y + 1, x) - AT(next, y - 1, x) - AT(prev, y + 1, x) + AT(prev, y - 1, x)) / 4.f;
        const float h13 = (AT(next, y, x + 1) - AT(next, y, x - 1) - AT(prev, y, x + 1) + AT(prev, y, x - 1)) / 4.f;
        const float h22 = AT(curr, y + 1, x) + AT(curr, y - 1, x) - v2;
        const float h33 = AT(curr, y, x + 1) + AT(curr, y, x - 1) - v2;
        const float h23 =
            (AT(curr, y + 1, x + 1) - AT(curr, y + 1, x - 1) - AT(curr, y - 1, x + 1) + AT(curr, y - 1, x - 1)) / 4.f;
#undef AT
        const float det =
            h11 * h22 * h33 - h11 * h23 * h23 - h12 * h12 * h33 + 2.f * h12 * h13 * h23 - h13 * h13 * h22;
        const float i11 = (h22 * h33 - h23 * h23) / det;
        const float i12 = (h13 * h23 - h12 * h33) / det;
        const float i13 = (h12 * h23 - h13 * h22) / det;
        const float i22 = (h11 * h33 - h13 * h13) / det;
        const float i23 = (h12 * h13 - h11 * h23) / det;
        const float i33 = (h11 * h22 - h12 * h12) / det;
        const float s_ = -(i11 * g1 + i12 * g2 + i13 * g3);
        const float x_ = -(i13 * g1 + i23 * g2 + i33 * g3);
        const float y_ = -(i12 * g1 + i22 * g2 + i23 * g3);
        if (fabsf(s_) < 0.5f && fabsf(x_) < 0.5f && fabsf(y_) < 0.5f) {
            os = s_;
            ox = x_;
            oy = y_;
            return true;
        }
        // `x as isize + offset.round() as isize` (saturating), then bounds
        const int64_t LIM = (int64_t)1 << 40;
        const int64_t rx = sat_i64(roundf(x_)), ry = sat_i64(roundf(y_)), rs = sat_i64(roundf(s_));
        if (rx > LIM || rx < -LIM || ry > LIM || ry < -LIM || rs > LIM || rs < -LIM) return false;
        const int64_t nx = x + rx, ny = y + ry, ns = scale + rs;
        if (!(ns >= 1 && ns <= kScalesPerOctave) || nx < kImageBorder || nx >= W - kImageBorder ||
            ny < kImageBorder || ny >= H - kImageBorder)
            return false;
        x = (int)nx;
        y = (int)ny;
        scale = (int)ns;
    }
    return false;
}

__device__ __forceinline__ bool refine_one_old(const RefineLaunch& L, uint64_t key, ExtRec& e) {
    const int b = (int)(key >> kKeyImgShift);
    const int o = (int)((key >> kKeyOctShift) & 15);
    const int s_in = (int)((key >> kKeyScaleShift) & 3);
    const int y = (int)((key >> kKeyYShift) & kKeyCoordMask);
    const int x = (int)((key >> kKeyXShift) & kKeyCoordMask);
    const int W = L.oct.ow[o], H = L.oct.oh[o], pitch = L.oct.opitch[o];
    const DogViewOld dv{as_global(L.oct.gauss[o]) + (size_t)(b - L.img_base) * L.oct.img_stride[o], (size_t)pitch * H};
    int sc = s_in, xi = x, yi = y;
    float os, ox, oy;
    int vlo = 0, vhi = H;  // rows of this octave's Gaussians that are exact
    if (L.band_flag) {
        vlo = max(0, (int)((uint64_t)H * L.band_r / L.band_n) - 1 - L.band_margin);
        vhi = min(H, (int)((uint64_t)H * (L.band_r + 1) / L.band_n) + 1 + L.band_margin);
    }
    if (!interpolate_old(dv, W, H, pitch, sc, xi, yi, os, ox, oy, L.band_flag, vlo, vhi)) return false;
    const size_t c = (size_t)yi * pitch + xi;
    auto prev = [&](size_t off) { return dv(sc - 1, off); };
    auto curr = [&](size_t off) { return dv(sc, off); };
    auto next = [&](size_t off) { return dv(sc + 1, off); };
    // extremum_contrast (src/lib.rs:606-626)
    const float g1 = (next(c) - prev(c)) / 2.f;
    const float g2 = (curr(c + pitch) - curr(c - pitch)) / 2.f;
    const float g3 = (curr(c + 1) - curr(c - 1)) / 2.f;
    const float interp = os * g1 + oy * g2 + ox * g3;
    const float contrast = fabsf(curr(c) + interp / 2.f);
    if (contrast * (float)kScalesPerOctave <= kContrastThreshold) return false;
    // extremum_is_on_edge (src/lib.rs:630-653)
    const float v2 = curr(c) * 2.0f;
    const float h11 = curr(c + pitch) + curr(c - pitch) - v2;
    const float d22 = curr(c + 1) + curr(c - 1) - v2;
    const float h12 = (curr(c + pitch + 1) - curr(c + pitch - 1) - curr(c - pitch + 1) + curr(c - pitch - 1)) / 4.f;
    const float tr = d22 + h11;
    const float det = d22 * h11 - h12 * h12;
    if (det <= 0.f) return false;
    if ((tr * tr * kEdgeThreshold) > (kEdgeThreshold + 1.0f) * (kEdgeThreshold + 1.0f) * det) return false;
    // an accepted keypoint's orientation / descriptor patch must be exact too
    // (at the image's own top / bottom rows the patch reads clamp, so no limit)
    if (L.band_flag && ((vlo > 0 && yi - L.band_patch < vlo) || (vhi < H && yi + L.band_patch >= vhi)))
        atomicOr(L.band_flag, 1u);
    e.key = key;
    e.img = b;
    e.octave = o;
    e.scale = sc;
    e.x = xi;
    e.y = yi;
    e.off_s = os;
    e.off_x = ox;
    e.off_y = oy;
    e.response = contrast;
    e.pad = 0;
    return true;
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SIFT_REFINE_WPE))) void k_refine_old(const RefineLaunch L) {
    const uint32_t n = min(*L.n_cand, L.cand_cap);
    const int lane = threadIdx.x & 63;
    for (uint32_t base = blockIdx.x * 256; base < n; base += gridDim.x * 256) {
        const uint32_t i = base + threadIdx.x;
        ExtRec e;
        const bool keep = i < n && refine_one_old(L, L.cand[i], e);
        const uint64_t mask = __ballot(keep);
        if (!mask) continue;
        const int leader = __ffsll((unsigned long long)mask) - 1;
        uint32_t b = 0;
        if (lane == leader) b = atomicAdd(L.counter, (uint32_t)__popcll(mask));
        b = __shfl(b, leader);
        const uint32_t slot = b + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (keep && slot < L.cap) L.out[slot] = e;
    }
}

// the first round-5 k_refine (one candidate per lane for its whole refinement), for A/B
// On success n holds the neighbourhood of the converged point (scale, y, x),
// which extremum_contrast / extremum_is_on_edge read next.
__device__ __forceinline__ bool interpolate_r5a(const gfloat* g0, size_t P, int W, int H, int pitch, int& scale, int& x,
                                            int& y, float& os, float& ox, float& oy, Nbhd& n, uint32_t* band_flag,
                                            int vlo, int vhi) {
    for (int it = 0; it < kMaxInterpSteps; it++) {
        // row bands with a restricted pyramid (pipeline.cpp PyramidRun): the
        // rows read here must be computed ones, else the host recomputes the
        // band on the whole-frame pyramid
        if (band_flag && (y - 1 < vlo || y + 1 >= vhi)) atomicOr(band_flag, 1u);
        load_nbhd(g0, P, pitch, scale, y, x, n);
        // AT(plane, dy, dx): plane 0 / 1 / 2 = prev / curr / next
#define AT(a, dy, dx) n.d[a][(dy) + 1][(dx) + 1]
        const float g1 = (AT(2, 0, 0) - AT(0, 0, 0)) / 2.f;
        const float g2 = (AT(1, 1, 0) - AT(1, -1, 0)) / 2.f;
        const float g3 = (AT(1, 0, 1) - AT(1, 0, -1)) / 2.f;
        const float v2 = AT(1, 0, 0) * 2.f;
        const float h11 = AT(2, 0, 0) + AT(0, 0, 0) - v2;
        const float h12 = (AT(2, 1, 0) - AT(2, -1, 0) - AT(0, 1, 0) + AT(0, -1, 0)) / 4.f;
        const float h13 = (AT(2, 0, 1) - AT(2, 0, -1) - AT(0, 0, 1) + AT(0, 0, -1)) / 4.f;
        const float h22 = AT(1, 1, 0) + AT(1, -1, 0) - v2;
        const float h33 = AT(1, 0, 1) + AT(1, 0, -1) - v2;
        const float h23 = (AT(1, 1, 1) - AT(1, 1, -1) - AT(1, -1, 1) + AT(1, -1, -1)) / 4.f;
#undef AT
        const float det =
            h11 * h22 * h33 - h11 * h23 * h23 - h12 * h12 * h33 + 2.f * h12 * h13 * h23 - h13 * h13 * h22;
        const float i11 = (h22 * h33 - h23 * h23) / det;
        const float i12 = (h13 * h23 - h12 * h33) / det;
        const float i13 = (h12 * h23 - h13 * h22) / det;
        const float i22 = (h11 * h33 - h13 * h13) / det;
        const float i23 = (h12 * h13 - h11 * h23) / det;
        const float i33 = (h11 * h22 - h12 * h12) / det;
        const float s_ = -(i11 * g1 + i12 * g2 + i13 * g3);
        const float x_ = -(i13 * g1 + i23 * g2 + i33 * g3);
        const float y_ = -(i12 * g1 + i22 * g2 + i23 * g3);
        if (fabsf(s_) < 0.5f && fabsf(x_) < 0.5f && fabsf(y_) < 0.5f) {
            os = s_;
            ox = x_;
            oy = y_;
            return true;
        }
        // `x as isize + offset.round() as isize` (saturating), then bounds
        const int64_t LIM = (int64_t)1 << 40;
        const int64_t rx = sat_i64(roundf(x_)), ry = sat_i64(roundf(y_)), rs = sat_i64(roundf(s_));
        if (rx > LIM || rx < -LIM || ry > LIM || ry < -LIM || rs > LIM || rs < -LIM) return false;
        const int64_t nx = x + rx, ny = y + ry, ns = scale + rs;
        if (!(ns >= 1 && ns <= kScalesPerOctave) || nx < kImageBorder || nx >= W - kImageBorder ||
            ny < kImageBorder || ny >= H - kImageBorder)
            return false;
        x = (int)nx;
        y = (int)ny;
        scale = (int)ns;
    }
    return false;
}

__device__ __forceinline__ bool refine_one_r5a(const RefineLaunch& L, uint64_t key, ExtRec& e) {
    const int b = (int)(key >> kKeyImgShift);
    const int o = (int)((key >> kKeyOctShift) & 15);
    const int s_in = (int)((key >> kKeyScaleShift) & 3);
    const int y = (int)((key >> kKeyYShift) & kKeyCoordMask);
    const int x = (int)((key >> kKeyXShift) & kKeyCoordMask);
    const int W = L.oct.ow[o], H = L.oct.oh[o], pitch = L.oct.opitch[o];
    const gfloat* g0 = as_global(L.oct.gauss[o]) + (size_t)(b - L.img_base) * L.oct.img_stride[o];
    const size_t P = (size_t)pitch * H;
    int sc = s_in, xi = x, yi = y;
    float os, ox, oy;
    Nbhd n;
    int vlo = 0, vhi = H;  // rows of this octave's Gaussians that are exact
    if (L.band_flag) {
        vlo = max(0, (int)((uint64_t)H * L.band_r / L.band_n) - 1 - L.band_margin);
        vhi = min(H, (int)((uint64_t)H * (L.band_r + 1) / L.band_n) + 1 + L.band_margin);
    }
    if (!interpolate_r5a(g0, P, W, H, pitch, sc, xi, yi, os, ox, oy, n, L.band_flag, vlo, vhi)) return false;
    // the converged point's neighbourhood is n (the last step did not move)
#define PREV(dy, dx) n.d[0][(dy) + 1][(dx) + 1]
#define CURR(dy, dx) n.d[1][(dy) + 1][(dx) + 1]
#define NEXT(dy, dx) n.d[2][(dy) + 1][(dx) + 1]
    // extremum_contrast (src/lib.rs:606-626)
    const float g1 = (NEXT(0, 0) - PREV(0, 0)) / 2.f;
    const float g2 = (CURR(1, 0) - CURR(-1, 0)) / 2.f;
    const float g3 = (CURR(0, 1) - CURR(0, -1)) / 2.f;
    const float interp = os * g1 + oy * g2 + ox * g3;
    const float contrast = fabsf(CURR(0, 0) + interp / 2.f);
    if (contrast * (float)kScalesPerOctave <= kContrastThreshold) return false;
    // extremum_is_on_edge (src/lib.rs:630-653)
    const float v2 = CURR(0, 0) * 2.0f;
    const float h11 = CURR(1, 0) + CURR(-1, 0) - v2;
    const float d22 = CURR(0, 1) + CURR(0, -1) - v2;
    const float h12 = (CURR(1, 1) - CURR(1, -1) - CURR(-1, 1) + CURR(-1, -1)) / 4.f;
#undef PREV
#undef CURR
#undef NEXT
    const float tr = d22 + h11;
    const float det = d22 * h11 - h12 * h12;
    if (det <= 0.f) return false;
    if ((tr * tr * kEdgeThreshold) > (kEdgeThreshold + 1.0f) * (kEdgeThreshold + 1.0f) * det) return false;
    // an accepted keypoint's orientation / descriptor patch must be exact too
    // (at the image's own top / bottom rows the patch reads clamp, so no limit)
    if (L.band_flag && ((vlo > 0 && yi - L.band_patch < vlo) || (vhi < H && yi + L.band_patch >= vhi)))
        atomicOr(L.band_flag, 1u);
    e.key = key;
    e.img = b;
    e.octave = o;
    e.scale = sc;
    e.x = xi;
    e.y = yi;
    e.off_s = os;
    e.off_x = ox;
    e.off_y = oy;
    e.response = contrast;
    e.pad = 0;
    return true;
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SIFT_REFINE_WPE))) void k_refine_r5a(const RefineLaunch L) {
    const uint32_t n = min(*L.n_cand, L.cand_cap);
    const int lane = threadIdx.x & 63;
    for (uint32_t base = blockIdx.x * 256; base < n; base += gridDim.x * 256) {
        const uint32_t i = base + threadIdx.x;
        ExtRec e;
        const bool keep = i < n && refine_one_r5a(L, L.cand[i], e);
        const uint64_t mask = __ballot(keep);
        if (!mask) continue;
        const int leader = __ffsll((unsigned long long)mask) - 1;
        uint32_t b = 0;
        if (lane == leader) b = atomicAdd(L.counter, (uint32_t)__popcll(mask));
        b = __shfl(b, leader);
        const uint32_t slot = b + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (keep && slot < L.cap) L.out[slot] = e;
    }
}

}  // namespace siftmi

#define CK(x)                                                                    \
    do {                                                                         \
        hipError_t e = (x);                                                      \
        if (e != hipSuccess) {                                                   \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e));          \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

// blobs (as sift-features_amd/synth.py: mid grey, ~300 Gaussian blobs of
// sigma 2..60 px per 1080p frame at 2x) + a gradient + a little noise, in
// [0, 1]; each 64 x 64 tile sums the blobs whose 3-sigma box reaches it
__device__ __forceinline__ uint32_t hsh(uint32_t h) {
    h ^= h >> 16;
    h *= 0x7feb352dU;
    h ^= h >> 15;
    h *= 0x846ca68bU;
    h ^= h >> 16;
    return h;
}
__device__ __forceinline__ float hf(uint32_t h) { return (float)(hsh(h) & 0xffffff) / 16777216.0f; }
constexpr int kBlobs = 300;
__global__ void k_fill_smooth(float* p, int W, int H, int pitch, size_t stride, int n) {
    __shared__ float bx[kBlobs], by[kBlobs], bs[kBlobs], ba[kBlobs];
    __shared__ int nb;
    const int f = blockIdx.z, tx = blockIdx.x * 64, ty = blockIdx.y * 64;
    if (threadIdx.x == 0) nb = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < kBlobs; k += 256) {
        const uint32_t s0 = (uint32_t)(f * kBlobs + k) * 4u;
        const float cx = hf(s0) * W, cy = hf(s0 + 1) * H, sg = 2.0f * (2.0f + 58.0f * hf(s0 + 2) * hf(s0 + 2));
        const float a = (hf(s0 + 3) - 0.5f) * 2.0f * 80.0f / 255.0f;
        if (cx + 3 * sg >= tx && cx - 3 * sg < tx + 64 && cy + 3 * sg >= ty && cy - 3 * sg < ty + 64) {
            const int i = atomicAdd(&nb, 1);
            bx[i] = cx, by[i] = cy, bs[i] = -0.5f / (sg * sg), ba[i] = a;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * 64; e += 256) {
        const int x = tx + (e & 63), y = ty + (e >> 6);
        if (x >= W || y >= H) continue;
        float v = 0.5f + 0.05f * (float)x / W - 0.05f * (float)y / H;
        for (int k = 0; k < nb; k++) {
            const float dx = x - bx[k], dy = y - by[k];
            v += ba[k] * __expf((dx * dx + dy * dy) * bs[k]);
        }
        v += (hf((uint32_t)(f * 7919 + y) * 65536u + x) - 0.5f) * 6.0f / 255.0f;
        p[(size_t)f * stride + (size_t)y * pitch + x] = fminf(fmaxf(v, 0.0f), 1.0f);
    }
}

template <class F>
float timeit(F f, int reps = 5) {
    f();
    CK(hipDeviceSynchronize());
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    CK(hipEventRecord(a));
    for (int i = 0; i < reps; i++) f();
    CK(hipEventRecord(b));
    CK(hipEventSynchronize(b));
    float ms;
    CK(hipEventElapsedTime(&ms, a, b));
    return ms / reps;
}

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 16;
    const int W = 3840, H = 2160, pitch = 3840;
    const size_t P = (size_t)pitch * H, stride = 6 * P;
    float* g = nullptr;
    CK(hipMalloc(&g, stride * n * sizeof(float)));
    hipLaunchKernelGGL(k_fill_smooth, dim3((W + 63) / 64, (H + 63) / 64, n), dim3(256), 0, 0, g, W, H, pitch, stride, n);
    // OpenCV octave sigmas (geometry.cpp octave_sigmas / cv_blur_taps): radii 5, 6, 8, 10, 13
    const double sig[6] = {0, 1.2262735, 1.5450078, 1.9465878, 2.4525469, 3.0900155};
    BlurTaps taps[6]{};
    int rad[6]{};
    for (int s = 1; s < 6; s++) {
        const int nn = ((int)std::lrint(sig[s] * 8 + 1)) | 1, r = nn / 2;
        const double scale2X = -0.125 / (sig[s] * sig[s]);
        double vals[64], sum = 0;
        for (int i = 0, x = 1 - nn; i < (nn - 1) / 2; i++, x += 2) {
            vals[i] = std::exp((double)(x * x) * scale2X);
            sum += vals[i];
        }
        sum = sum * 2 + 1;
        taps[s].k[0] = (float)(1.0 / sum);
        for (int i = 0; i < (nn - 1) / 2; i++) taps[s].k[r - i] = (float)(vals[i] / sum);
        rad[s] = r;
    }
    auto blur = [&](int s) {
        BlurLaunch B{};
        B.src = g + (size_t)(s - 1) * P;
        B.src_img_stride = stride;
        B.dst = g + (size_t)s * P;
        B.dst_img_stride = stride;
        B.W = W;
        B.H = H;
        B.pitch = pitch;
        B.n_img = n;
        B.taps = taps[s];
        B.profile = kProfileOpenCV;
        return B;
    };
    for (int s = 1; s < 6; s++) CK((hipError_t)launch_blur(rad[s], blur(s), 0));
    CK(hipDeviceSynchronize());
    const double px = (double)W * H * n;
    uint64_t* cand = nullptr;
    uint32_t* cnt = nullptr;
    const uint32_t cap = 1u << 26;
    CK(hipMalloc(&cand, cap * sizeof(uint64_t)));
    CK(hipMalloc(&cnt, 64));
    const float t4 = timeit([&] { launch_blur(rad[4], blur(4), 0); });
    const float t5 = timeit([&] { launch_blur(rad[5], blur(5), 0); });
    DetectLaunch D{};
    D.n_img = n;
    D.cand = cand;
    D.counter = cnt;
    D.cap = cap;
    D.n_oct = 1;
    D.oct[0].gauss = g;
    D.oct[0].img_stride = stride;
    D.oct[0].W = W;
    D.oct[0].H = H;
    D.oct[0].pitch = pitch;
    D.oct[0].y_lo = 0;
    D.oct[0].y_hi = H;
    const float td = timeit([&] {
        CK(hipMemsetAsync(cnt, 0, 4, 0));
        DetectLaunch d = D;
        launch_detect(d, 0);
    });
    uint32_t nc_rows = 0;
    CK(hipMemcpy(&nc_rows, cnt, 4, hipMemcpyDeviceToHost));
    std::vector<uint64_t> c_rows(nc_rows);
    CK(hipMemcpy(c_rows.data(), cand, nc_rows * 8, hipMemcpyDeviceToHost));
    std::sort(c_rows.begin(), c_rows.end());
    // G_5 of the strip blur (frame 0 and the last), to compare with k_blur_detect's
    std::vector<float> g5a(P), g5b(P), g5c(P), g5d(P);
    CK(hipMemcpy(g5a.data(), g + 5 * P, P * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(g5b.data(), g + (size_t)(n - 1) * stride + 5 * P, P * 4, hipMemcpyDeviceToHost));
    BlurDetectLaunch F{};
    F.gauss = g;
    F.img_stride = stride;
    F.W = W;
    F.H = H;
    F.pitch = pitch;
    F.n_img = n;
    F.profile = kProfileOpenCV;
    F.taps = taps[5];
    F.cand = cand;
    F.counter = cnt;
    F.cap = cap;
    const float tbd = timeit([&] {
        CK(hipMemsetAsync(cnt, 0, 4, 0));
        BlurDetectLaunch f = F;
        launch_blur_detect(rad[5], f, 0);
    });
    // the pair kernel (two column strips per lane): time, then G_5 and candidates
    const int bdw = getenv("BD_WAVES") ? atoi(getenv("BD_WAVES")) : 8192;
    for (int mode = 1; mode <= 1; mode++) {
    PathOpts po2{};
    po2.bd_pair = mode;
    po2.bd_waves = bdw;
    CK(hipMemset(g + 5 * P, 0, P * 4));
    const float tbp = timeit([&] {
        CK(hipMemsetAsync(cnt, 0, 4, 0));
        BlurDetectLaunch f = F;
        launch_blur_detect(rad[5], f, 0, po2);
    });
    {
        uint32_t np = 0;
        CK(hipMemcpy(&np, cnt, 4, hipMemcpyDeviceToHost));
        std::vector<uint64_t> c_p(np);
        CK(hipMemcpy(c_p.data(), cand, np * 8, hipMemcpyDeviceToHost));
        std::sort(c_p.begin(), c_p.end());
        std::vector<float> g5e(P), g5f(P);
        CK(hipMemcpy(g5e.data(), g + 5 * P, P * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(g5f.data(), g + (size_t)(n - 1) * stride + 5 * P, P * 4, hipMemcpyDeviceToHost));
        const bool sg = std::memcmp(g5a.data(), g5e.data(), P * 4) == 0 && std::memcmp(g5b.data(), g5f.data(), P * 4) == 0;
        BlurDetectLaunch f = F;
        launch_blur_detect(rad[5], f, 0, po2);  // fills nsx / seg for the report
        std::printf("k_blur_detect_pair%d  %8.1f us  %5.2f TB/s (24 B/px)  %u candidates  seg %d  G_5 %s, candidates %s\n",
                    mode, tbp * 1e3, 6 * (double)W * H * n * 4 / 1e6 / tbp / 1e3, np, f.seg,
                    sg ? "bit-identical" : "DIFFER", c_p == c_rows ? "identical" : "DIFFER");
        if (!sg || c_p != c_rows) {
            size_t bad = 0, first = 0;
            for (size_t i = 0; i < P; i++)
                if (g5a[i] != g5e[i]) { if (!bad) first = i; bad++; }
            std::printf("  G_5 frame 0: %zu differ, first at y %zu x %zu (%g vs %g)\n", bad, first / pitch, first % pitch,
                        bad ? g5a[first] : 0.f, bad ? g5e[first] : 0.f);
            return 5;
        }
    }
    }
    CK(hipDeviceSynchronize());
    {
        // restore k_blur_detect's outputs for the refine comparisons below
        CK(hipMemsetAsync(cnt, 0, 4, 0));
        BlurDetectLaunch f = F;
        launch_blur_detect(rad[5], f, 0);
    }
    uint32_t nc = 0;
    CK(hipMemcpy(&nc, cnt, 4, hipMemcpyDeviceToHost));
    std::vector<uint64_t> c_bd(nc);
    CK(hipMemcpy(c_bd.data(), cand, nc * 8, hipMemcpyDeviceToHost));
    const std::vector<uint64_t> c_raw = c_bd;  // k_blur_detect's append order
    std::sort(c_bd.begin(), c_bd.end());
    CK(hipMemcpy(g5c.data(), g + 5 * P, P * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(g5d.data(), g + (size_t)(n - 1) * stride + 5 * P, P * 4, hipMemcpyDeviceToHost));
    const bool same_g5 = std::memcmp(g5a.data(), g5c.data(), P * 4) == 0 && std::memcmp(g5b.data(), g5d.data(), P * 4) == 0;
    const bool same_cand = c_rows == c_bd;
    // refine the candidates, in sorted and in k_blur_detect's append order
    const float** dg = nullptr;
    size_t* dgs = nullptr;
    int *dw = nullptr, *dh = nullptr, *dp = nullptr;
    CK(hipMalloc(&dg, sizeof(float*)));
    CK(hipMalloc(&dgs, sizeof(size_t)));
    CK(hipMalloc(&dw, 4));
    CK(hipMalloc(&dh, 4));
    CK(hipMalloc(&dp, 4));
    const float* g0 = g;
    CK(hipMemcpy(dg, &g0, sizeof(float*), hipMemcpyHostToDevice));
    CK(hipMemcpy(dgs, &stride, sizeof(size_t), hipMemcpyHostToDevice));
    CK(hipMemcpy(dw, &W, 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dh, &H, 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dp, &pitch, 4, hipMemcpyHostToDevice));
    nc = nc_rows;
    ExtRec* ext = nullptr;
    CK(hipMalloc(&ext, (size_t)nc * sizeof(ExtRec) + 64));
    RefineLaunch R{};
    R.cand = cand;
    R.n_cand = cnt;
    R.cand_cap = nc;
    R.oct = OctaveView{dg, dgs, dw, dh, dp};
    R.n_oct = 1;
    R.out = ext;
    R.counter = cnt + 1;
    R.cap = nc;
    R.band_n = 1;
    // the same extrema (the append order differs run to run): sort by key
    auto fetch_sorted = [&]() {
        uint32_t ne = 0;
        CK(hipMemcpy(&ne, cnt + 1, 4, hipMemcpyDeviceToHost));
        std::vector<ExtRec> v(ne);
        CK(hipMemcpy(v.data(), ext, ne * sizeof(ExtRec), hipMemcpyDeviceToHost));
        std::sort(v.begin(), v.end(), [](const ExtRec& a, const ExtRec& b) { return a.key < b.key; });
        return v;
    };
    const uint32_t grid = std::min<uint32_t>((R.cand_cap + 255) / 256, 2048);
    bool same = true;
    const std::vector<uint64_t>* orders[2] = {&c_rows, &c_raw};
    const char* oname[2] = {"sorted", "append order"};
    std::printf("octave 0 of %d 1080p frames (%.0f M px)\n", n, px / 1e6);
    for (int k = 0; k < 2; k++) {
        CK(hipMemcpy(cand, orders[k]->data(), nc * 8, hipMemcpyHostToDevice));
        CK(hipMemcpy(cnt, &nc, 4, hipMemcpyHostToDevice));
        const float tr = timeit([&] {
            CK(hipMemsetAsync(cnt + 1, 0, 4, 0));
            launch_refine(R, 0);
        });
        const std::vector<ExtRec> e_new = fetch_sorted();
        const float tr5 = timeit([&] {
            CK(hipMemsetAsync(cnt + 1, 0, 4, 0));
            hipLaunchKernelGGL(k_refine_r5a, dim3(grid), dim3(256), 0, 0, R);
        });
        const std::vector<ExtRec> e_r5 = fetch_sorted();
        const float tro = timeit([&] {
            CK(hipMemsetAsync(cnt + 1, 0, 4, 0));
            hipLaunchKernelGGL(k_refine_old, dim3(grid), dim3(256), 0, 0, R);
        });
        const std::vector<ExtRec> e_old = fetch_sorted();
        auto eq = [](const std::vector<ExtRec>& a, const std::vector<ExtRec>& b) {
            return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(ExtRec)) == 0;
        };
        const bool s1 = eq(e_new, e_old), s2 = eq(e_r5, e_old);
        same = same && s1 && s2;
        std::printf("k_refine (%s)    %8.1f us  %u candidates -> %zu extrema; identical to round 4: %s\n", oname[k],
                    tr * 1e3, nc, e_new.size(), s1 ? "yes" : "NO");
        std::printf("k_refine r5a (%s) %8.1f us  identical: %s\n", oname[k], tr5 * 1e3, s2 ? "yes" : "NO");
        std::printf("k_refine r4 (%s)  %8.1f us\n", oname[k], tro * 1e3);
    }
    const double mb = px * 4 / 1e6;  // MB per plane over the batch (MB / ms / 1e3 = TB/s)
    std::printf("blur4 strip R=%d     %8.1f us  %5.2f TB/s (8 B/px)\n", rad[4], t4 * 1e3, 2 * mb / t4 / 1e3);
    std::printf("blur5 strip R=%d     %8.1f us  %5.2f TB/s (8 B/px)\n", rad[5], t5 * 1e3, 2 * mb / t5 / 1e3);
    std::printf("k_detect_rows        %8.1f us  %5.2f TB/s (24 B/px)  %u candidates\n", td * 1e3,
                6 * mb / td / 1e3, nc_rows);
    std::printf("k_blur_detect        %8.1f us  %5.2f TB/s (24 B/px)  %u candidates\n", tbd * 1e3,
                6 * mb / tbd / 1e3, (unsigned)c_raw.size());
    std::printf("blur5 + detect_rows  %8.1f us\n", (t5 + td) * 1e3);
    std::printf("k_blur_detect vs strip blur 5 + k_detect_rows: G_5 %s, candidates %s\n",
                same_g5 ? "bit-identical" : "DIFFER", same_cand ? "identical" : "DIFFER");
    if (!same_g5 || !same_cand) return 4;
    return same ? 0 : 3;
}
