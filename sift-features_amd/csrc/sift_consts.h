// Constants and records shared by host-only code (geometry.cpp) and the HIP
// sources: nothing here needs the HIP headers.
#pragma once

namespace siftmi {

constexpr int kScalesPerOctave = 3;                  // src/lib.rs:92
constexpr int kImagesPerOctave = kScalesPerOctave + 3;  // 6 Gaussian images (src/lib.rs:218-221)
constexpr int kDogPerOctave = kScalesPerOctave + 2;     // 5 DoG images (src/lib.rs:277)
constexpr int kMaxBlurRadius = 31;                   // taps <= 63 per pass

// Blur taps, centre-indexed: k[0] = centre, k[t] = tap at distance t.
struct BlurTaps {
    float k[kMaxBlurRadius + 1];
};

}  // namespace siftmi
