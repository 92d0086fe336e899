// Stand-alone driver of sift-features_amd/csrc/geometry.cpp for
// tests/test_host_geometry.py: prints what the host arithmetic computes, one
// record per line, floats as hex floats (compared bit for bit).  Built with
// the host compiler and -fsanitize=address,undefined.
#include <cstdio>
#include <vector>

#include "geometry.h"

using namespace siftmi;

static const int kFrames[][2] = {{1, 1}, {2, 3}, {16, 16}, {97, 161}, {640, 480}, {1920, 1080}, {8192, 8192}, {16384, 1}};

static void print_taps(const char* tag, double sigma, int r, const BlurTaps& t) {
    std::printf("%s %a %d", tag, sigma, r);
    for (int i = 0; i <= r; i++) std::printf(" %a", (double)t.k[i]);
    std::printf("\n");
}

int main() {
    for (auto& f : kFrames) std::printf("n_octaves %d %d %d\n", f[0], f[1], n_octaves_for(f[0], f[1]));

    double sig[kImagesPerOctave];
    octave_sigmas(sig);
    std::printf("octave_sigmas");
    for (double s : sig) std::printf(" %a", s);
    std::printf("\nseed_sigma %a\n", seed_sigma());

    // taps of the seed blur and the five octave blurs, both profiles
    // (ImageprocProcessing takes sigma as f32)
    int oct_r[kImagesPerOctave] = {};
    for (int s = 0; s < kImagesPerOctave; s++) {
        const double sigma = s == 0 ? seed_sigma() : sig[s];
        BlurTaps t;
        const int r = cv_blur_taps(sigma, &t);
        if (s) oct_r[s] = r;
        print_taps("cv_taps", sigma, r, t);
        print_taps("ip_taps", (double)(float)sigma, ip_blur_taps((float)sigma, &t), t);
    }

    // the 2x Triangle upsample and the nearest 1/2, odd and even source sizes
    const struct { int src, dst; float support; } axes[] = {{97, 194, 1.0f}, {16, 32, 1.0f}, {97, 48, 0.0f}, {16, 8, 0.0f}};
    for (auto& a : axes)
        for (int o = 0; o < a.dst; o++) {
            int left = 0;
            float w[64];
            const int n = ip_axis(a.src, a.dst, o, a.support, &left, w);
            std::printf("ip_axis %d %d %a %d %d %d", a.src, a.dst, (double)a.support, o, left, n);
            for (int i = 0; i < n; i++) std::printf(" %a", (double)w[i]);
            std::printf("\n");
        }

    // octave geometry (one frame per chunk) and the nearest 1/2 check
    for (auto& f : kFrames) {
        OctaveGeom g;
        const int n_oct = n_octaves_for(f[0], f[1]);
        const bool ok = octave_geometry(f[0], f[1], n_oct, 1, g);
        std::printf("geometry %d %d %d %zu\n", f[0], f[1], ok ? 1 : 0, ok ? g.arena_floats : (size_t)0);
        for (int o = 0; ok && o < n_oct; o++)
            std::printf("octave %d %d %d %d %d %d %zu %zu %zu %zu %d %d\n", f[0], f[1], o, g.ow[o], g.oh[o], g.opitch[o],
                        g.P[o], g.px[o], g.goff[o], g.doff[o], nearest_half_check(g.ow[o], false),
                        nearest_half_check(g.oh[o], true));
    }

    // row bands over the octave heights of two frames, with the OpenCV radii
    const int band_frames[][2] = {{97, 161}, {1920, 1080}};
    for (auto& f : band_frames) {
        OctaveGeom g;
        const int n_oct = n_octaves_for(f[0], f[1]);
        if (!octave_geometry(f[0], f[1], n_oct, 1, g)) return 1;
        for (int band_n : {1, 2, 3, 8})
            for (int band_r = 0; band_r < band_n; band_r++) {
                const BandRows R = band_rows(g.oh.data(), n_oct, oct_r, band_r, band_n);
                for (int o = 0; o < n_oct; o++) {
                    std::printf("band %d %d %d %d %d %d %d %d", f[0], f[1], band_n, band_r, o, g.oh[o],
                                band_row_lo(g.oh[o], band_r, band_n), band_row_hi(g.oh[o], band_r, band_n));
                    for (int s = 0; s < kImagesPerOctave; s++)
                        std::printf(" %d %d", R.lo[(size_t)o * kImagesPerOctave + s], R.hi[(size_t)o * kImagesPerOctave + s]);
                    std::printf("\n");
                }
            }
    }
    std::printf("band_radii");
    for (int s = 1; s < kImagesPerOctave; s++) std::printf(" %d", oct_r[s]);
    std::printf("\n");

    for (int mode : {1, 0}) {
        std::printf("auto_chunk 1920 1080 128 %d %u\n", mode, auto_chunk(1920, 1080, 128, mode, 0));
        std::printf("auto_chunk 640 480 256 %d %u\n", mode, auto_chunk(640, 480, 256, mode, 0));
    }
    return 0;
}
