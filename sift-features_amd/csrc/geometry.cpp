// Reference host arithmetic (geometry.h).  Build with -ffp-contract=off.
#include "geometry.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace siftmi {

// n_octaves = round(log2(min(2W,2H)) - 2) as usize + 1  (src/lib.rs:133-134)
int n_octaves_for(uint32_t w, uint32_t h) {
    const uint32_t m = std::min(2 * w, 2 * h);
    const float f = roundf(log2f((float)m) - 2.0f);
    const size_t u = (f > 0.0f) ? (size_t)f : 0;  // saturating `as usize`
    return (int)u + 1;
}

double powi_f64(double a, int b) {  // compiler-rt __powidf2 (llvm.powi)
    const bool recip = b < 0;
    double r = 1;
    for (;;) {
        if (b & 1) r *= a;
        b /= 2;
        if (b == 0) break;
        a *= a;
    }
    return recip ? 1 / r : r;
}

// src/lib.rs:220-229
void octave_sigmas(double* sig) {
    const double m = std::pow(2.0, 2.0 / kScalesPerOctave);
    for (int s = 0; s < kImagesPerOctave; s++) {
        const double a = powi_f64(m, s - 1);
        const double b = a * m;
        sig[s] = std::sqrt(b - a) * 0.8 * 2.0;
    }
}
// src/lib.rs:207
double seed_sigma() { return std::sqrt(0.8 * 0.8 - 0.5 * 0.5) * 2.0; }

// cv::GaussianBlur(Size(), sigma), CV_32F: ksize = cvRound(sigma*4*2+1)|1;
// taps from getGaussianKernelBitExact (IEEE double), cast to f32.
int cv_blur_taps(double sigma, BlurTaps* t) {
    const int n = ((int)std::lrint(sigma * 4 * 2 + 1)) | 1;
    const int r = n / 2;
    if (r < 1 || r > 24) return -1;
    const double scale2X = -0.125 / (sigma * sigma);
    const int n2 = (n - 1) / 2;
    double values[64];
    double sum = 0;
    for (int i = 0, x = 1 - n; i < n2; i++, x += 2) {
        const double v = std::exp((double)(x * x) * scale2X);
        values[i] = v;
        sum += v;
    }
    sum *= 2;
    sum += 1;
    const double mul1 = 1 / sum;
    std::memset(t, 0, sizeof(*t));
    t->k[0] = (float)(1.0 * mul1);
    for (int i = 0; i < n2; i++) t->k[r - i] = (float)(values[i] * mul1);
    return r;
}

// cv::resize INTER_LINEAR coefficient table (resizeGeneric_)
void cv_linear_coeffs(int ssz, int dsz, std::vector<int>& ofs, std::vector<float>& a0, std::vector<float>& a1,
                      int* lim) {
    const double inv = (double)dsz / ssz;
    const double scale = 1. / inv;
    int xmax = dsz;
    ofs.resize(dsz);
    a0.resize(dsz);
    a1.resize(dsz);
    for (int d = 0; d < dsz; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)floorf(f);
        f -= (float)s;
        if (s < 0) {
            f = 0;
            s = 0;
        }
        if (s + 1 >= ssz) {
            if (d < xmax) xmax = d;
            if (s >= ssz - 1) {
                f = 0;
                s = ssz - 1;
            }
        }
        ofs[d] = s;
        a0[d] = 1.f - f;
        a1[d] = f;
    }
    *lim = xmax;
}

// cv::resize INTER_NEAREST offsets (resizeNN)
void cv_nearest_ofs(int ssz, int dsz, std::vector<int>& ofs) {
    const double ifx = 1. / ((double)dsz / ssz);
    ofs.resize(dsz);
    for (int d = 0; d < dsz; d++) {
        const int s = (int)std::floor(d * ifx);
        ofs[d] = std::min(s, ssz - 1);
    }
}

// ---- ImageprocProcessing profile (src/lib.rs:993-1007) ---------------------
// imageproc 0.25.0 gaussian_kernel_f32 and image 0.25.2 imageops::resize
// sampling weights, restated (third-party code the reference depends on;
// parity unpinned -- DESIGN.md).  Same f32 arithmetic as oracle/sift_oracle.c.
int ip_blur_taps(float sigma, BlurTaps* t) {
    const int r = (int)std::ceil(2.0f * sigma);
    if (r < 1 || r > 24) return -1;
    const int n = 2 * r + 1;
    float k[64];
    const float norm = 1.0f / (std::sqrt(2.0f * 3.14159265358979323846f) * sigma);
    for (int i = 0; i <= r; i++) {
        const float x = (float)i;
        const float v = norm * std::exp(-(x * x) / (2.0f * (sigma * sigma)));
        k[r + i] = v;
        k[r - i] = v;
    }
    float sum = 0.0f;
    for (int i = 0; i < n; i++) sum += k[i];
    std::memset(t, 0, sizeof(*t));
    for (int i = 0; i <= r; i++) t->k[i] = k[r + i] / sum;
    return r;
}

int ip_axis(int src, int dst, int out, float support, int* left, float* w) {
    const float ratio = (float)src / (float)dst;
    const float sratio = ratio < 1.0f ? 1.0f : ratio;
    const float src_support = support * sratio;
    float in = ((float)out + 0.5f) * ratio;
    long l = (long)std::floor(in - src_support);
    l = l < 0 ? 0 : (l > src - 1 ? src - 1 : l);
    long rt = (long)std::ceil(in + src_support);
    rt = rt < l + 1 ? l + 1 : (rt > src ? src : rt);
    in = in - 0.5f;
    float sum = 0.0f;
    int n = 0;
    for (long i = l; i < rt; i++) {
        float v = 1.0f;  // box_kernel
        if (support > 0.0f) {
            const float a = std::fabs(((float)i - in) / sratio);
            v = a < 1.0f ? 1.0f - a : 0.0f;
        }
        w[n++] = v;
        sum += v;
    }
    for (int i = 0; i < n; i++) w[i] = w[i] / sum;
    *left = (int)l;
    return n;
}

bool octave_geometry(uint32_t w, uint32_t h, int n_oct, uint32_t chunk, OctaveGeom& g) {
    g.n_oct = n_oct;
    g.ow.assign(n_oct, 0);
    g.oh.assign(n_oct, 0);
    g.opitch.assign(n_oct, 0);
    g.P.assign(n_oct, 0);
    g.px.assign(n_oct, 0);
    g.goff.assign(n_oct, 0);
    g.doff.assign(n_oct, 0);
    g.sum_px = 0;
    int ow = 2 * (int)w, oh = 2 * (int)h;
    size_t total = 0;
    for (int o = 0; o < n_oct; o++) {
        if (ow < 1 || oh < 1) return false;
        g.ow[o] = ow;
        g.oh[o] = oh;
        g.opitch[o] = (ow + 63) & ~63;  // 256-B aligned rows
        g.P[o] = (size_t)g.opitch[o] * oh;
        g.px[o] = (size_t)ow * oh;
        g.sum_px += g.px[o];
        g.goff[o] = total;
        total += (size_t)chunk * kImagesPerOctave * g.P[o];
        g.doff[o] = total;
        // D_0..D_4 for ONE frame: only precompute_images materialises the
        // DoG (run_pyramid's `full`, one frame on lane 0); the batch path
        // forms D where it reads it.  (Rounds 1-5 reserved them per chunk
        // frame: 5 / 11 of the arena never written -- 28 GB per lane at 128 x
        // 1080p.)
        total += (size_t)kDogPerOctave * g.P[o];
        total = (total + 63) & ~(size_t)63;  // 256-B aligned octave arenas
        ow /= 2;
        oh /= 2;
    }
    g.arena_floats = total;
    return true;
}

int nearest_half_check(int src, bool imageproc) {
    const int dst = src / 2, par = imageproc ? 1 : 0;
    std::vector<int> xo;
    if (imageproc) {
        xo.resize(dst);
        float wt[8];
        for (int i = 0; i < dst; i++)
            if (ip_axis(src, dst, i, 0.0f, &xo[i], wt) != 1) return 1;
    } else {
        cv_nearest_ofs(src, dst, xo);
    }
    for (int i = 0; i < dst; i++)
        if (xo[i] != 2 * i + par) return 2;
    return 0;
}

// The rows of every Gaussian the band's keypoint stages read, propagated back
// through the blur chain and the octave downsampling.  Detection covers
// octave rows [H*r/n, H*(r+1)/n); around them a margin of kBandDrift + 1 +
// kBandPatch rows.  Blur s reads oct_r[s] rows of G_{s-1} on either side, and
// octave o + 1's G_0 row y is G_3's row 2y or 2y + 1 of octave o.
BandRows band_rows(const int* oh, int n_oct, const int* oct_r, uint32_t band_r, uint32_t band_n) {
    BandRows R;
    R.lo.assign((size_t)n_oct * kImagesPerOctave, 0);
    R.hi.assign((size_t)n_oct * kImagesPerOctave, 0);
    int need_lo = 0, need_hi = 0;  // octave o + 1's G_0 rows, in octave o + 1 coordinates
    for (int o = n_oct - 1; o >= 0; o--) {
        const int H = oh[o], M = kBandDrift + 1 + kBandPatch;
        const int blo = band_row_lo(H, band_r, band_n), bhi = band_row_hi(H, band_r, band_n);
        int* lo = &R.lo[(size_t)o * kImagesPerOctave];
        int* hi = &R.hi[(size_t)o * kImagesPerOctave];
        for (int s = 0; s < kImagesPerOctave; s++) {
            lo[s] = blo - 1 - M;
            hi[s] = bhi + 1 + M;
        }
        if (o + 1 < n_oct && need_hi > need_lo) {  // nearest 1/2 of G_3: row 2y or 2y + 1
            lo[3] = std::min(lo[3], 2 * need_lo);
            hi[3] = std::max(hi[3], 2 * need_hi + 1);
        }
        for (int s = kImagesPerOctave - 1; s >= 1; s--) {
            lo[s - 1] = std::min(lo[s - 1], lo[s] - oct_r[s]);
            hi[s - 1] = std::max(hi[s - 1], hi[s] + oct_r[s]);
        }
        for (int s = 0; s < kImagesPerOctave; s++) {
            lo[s] = std::max(lo[s], 0);
            hi[s] = std::min(hi[s], H);
        }
        need_lo = lo[0];
        need_hi = hi[0];
    }
    return R;
}

uint32_t auto_chunk(uint32_t w, uint32_t h, uint32_t n, int mode, double avail_bytes) {
    // mode 1 (path option chunk_mode, the default since round 6): twice the
    // caps below and no forced second chunk -- a 128-frame 1080p call is one
    // chunk.  Against mode 0's two overlapped 64-frame chunks: 34.49-34.53 vs
    // 34.12-34.43 M keypoints/s, VGA 256 30.32-30.43 vs 30.00-30.21 M
    // (profiles/r06_ab_runs.md): each stage's launches twice as large beat
    // the overlap of two half-size chunks.
    // Up to ~32 GB of pyramid per chunk (two lanes: ~64 GB of the 288 GB HBM)
    // and at most kMaxChunk frames, in balanced chunks, at least two when the
    // batch has two frames (the lanes overlap consecutive chunks).  Bigger
    // chunks amortise each stage's launch tail: 1080p, 128 frames per call,
    // measured 22.8 M keypoints/s at 32-frame chunks, 23.9 M at 64.
    double sum_p = 0;
    uint32_t ow = 2 * w, oh = 2 * h;
    const int no = n_octaves_for(w, h);
    for (int o = 0; o < no; o++) {
        sum_p += (double)ow * oh;
        ow /= 2;
        oh /= 2;
    }
    // 44 B per octave pixel: every image of PrecomputedImages (6 G + 5 D).
    // The arena itself now costs 24 B per pixel per chunk frame (G_0..G_5)
    // plus one frame of DoG (octave_geometry); 44 B is kept as margin for the
    // stage buffers and whatever else the device holds.
    const double per_frame = 44.0 * sum_p;
    const double scale = mode == 1 ? 2.0 : 1.0;
    uint32_t cmax = (uint32_t)std::max(1.0, std::floor(scale * 32e9 / per_frame));
    // and at most 40% of the device memory this context could use (free +
    // its own arenas) per chunk: the two lanes' arenas stay below 80% however
    // much other work holds (no effect on an idle 288 GB MI355X)
    if (avail_bytes > 0) cmax = std::min<uint32_t>(cmax, (uint32_t)std::max(1.0, std::floor(0.4 * avail_bytes / per_frame)));
    // and ~531 M seed pixels (64 frames at 1080p): smaller frames get more
    // frames per chunk, so their octave launches are as large (VGA: 256
    // frames in two chunks of 128 instead of four of 64)
    const double seed_px = 4.0 * w * h;
    cmax = std::min<uint32_t>(cmax, (uint32_t)std::max(1.0, std::floor(scale * 64.0 * 3840.0 * 2160.0 / seed_px)));
    cmax = std::min<uint32_t>(cmax, 256);
    uint32_t k = std::max<uint32_t>((n + cmax - 1) / cmax, (n >= 2 && mode != 1) ? 2u : 1u);  // chunks
    return std::max<uint32_t>(1, (n + k - 1) / k);
}

}  // namespace siftmi
