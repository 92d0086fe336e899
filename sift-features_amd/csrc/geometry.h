// Host arithmetic that feeds the device, computed exactly as the reference /
// OpenCV / image compute it (IEEE double / f32, glibc libm): octave count,
// blur sigmas and taps, resize tables, the pyramid arena layout, the rows of a
// row band and the automatic chunk size.  No HIP here: the file builds with
// the host compiler alone (tests/test_host_geometry.py).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "sift_consts.h"

namespace siftmi {

int n_octaves_for(uint32_t w, uint32_t h);
double powi_f64(double a, int b);
void octave_sigmas(double* sig);  // sig[kImagesPerOctave]
double seed_sigma();

// Taps of one blur; returns its radius, -1 outside 1..24.
int cv_blur_taps(double sigma, BlurTaps* t);
int ip_blur_taps(float sigma, BlurTaps* t);

void cv_linear_coeffs(int ssz, int dsz, std::vector<int>& ofs, std::vector<float>& a0, std::vector<float>& a1,
                      int* lim);
void cv_nearest_ofs(int ssz, int dsz, std::vector<int>& ofs);
// One axis of image's vertical_sample / horizontal_sample: taps [left, left+n)
// with normalised f32 weights; support 1 = Triangle, 0 = Nearest.
int ip_axis(int src, int dst, int out, float support, int* left, float* w);

// Octave dimensions and the float offsets of one lane's pyramid arena
// [G_0 | D_0 | G_1 | D_1 ...] for `chunk` frames.
struct OctaveGeom {
    int n_oct = 0;
    std::vector<int> ow, oh, opitch;
    std::vector<size_t> P;           // floats per octave image plane (pitch * H)
    std::vector<size_t> px;          // real pixels per octave image (W * H)
    std::vector<size_t> goff, doff;  // float offsets of octave arenas
    size_t arena_floats = 0;
    uint64_t sum_px = 0;
};
// false: the image is too small for n_oct octaves
bool octave_geometry(uint32_t w, uint32_t h, int n_oct, uint32_t chunk, OctaveGeom& g);
// The fused nearest 1/2 of a src-long axis picks source pixel 2x (OpenCV
// INTER_NEAREST) or 2x + 1 (image Nearest).  0: it does; 1: image's sampler
// has more than one tap; 2: another offset.
int nearest_half_check(int src, bool imageproc);

// Row bands with a restricted pyramid: rows a refined keypoint may drift from
// its detection row and still be exact without a re-run, and the rows its
// orientation / descriptor patch reaches (radius <= 16 / 39, plus the
// gradient's neighbour row).
constexpr int kBandDrift = 24, kBandPatch = 41;

// Rows [lo, hi) of Gaussian s of octave o (index o * kImagesPerOctave + s)
// that band band_r of band_n needs.
struct BandRows {
    std::vector<int> lo, hi;
};
BandRows band_rows(const int* oh, int n_oct, const int* oct_r, uint32_t band_r, uint32_t band_n);
// the detection rows of that band in an octave of H rows: the bands of one
// octave partition [0, H)
inline int band_row_lo(int H, uint32_t band_r, uint32_t band_n) { return (int)((uint64_t)H * band_r / band_n); }
inline int band_row_hi(int H, uint32_t band_r, uint32_t band_n) { return (int)((uint64_t)H * (band_r + 1) / band_n); }

// Frames per chunk of an n-frame call (avail_bytes = 0: no memory cap).
uint32_t auto_chunk(uint32_t w, uint32_t h, uint32_t n, int mode, double avail_bytes);

}  // namespace siftmi
