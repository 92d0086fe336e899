// The JPEG step's host code (sift-features_amd/csrc/jpeg.hip: parse, geometry,
// check_support, entropy_decode) as a stand-alone program, for
// tests/test_jpeg_streams_cpu.py to build under AddressSanitizer and UBSan and
// run as a subprocess.  It makes no HIP call.
//   jpeg_host corpus
// `corpus` is a sequence of streams, each a 32-bit little-endian length and
// that many bytes.  Every stream is copied into a malloc block of exactly its
// length, so a read past its end is a report, and decoded the way
// jpeg_decode_luma does up to the upload.  Per stream:
//   stream <index> <status> <error text>
// and for status 0
//   frame <w> <h> <nc> <hmax> <vmax> <mcux> <mcuy>
//   comp <k> <id> <h> <v> <tq> <td> <ta> <blocks per row> <blocks per column>
//   q <k> <64 table entries, natural order>
//   coef <k> <every quantised coefficient of the plane, block by block, natural order>
#include "../sift-features_amd/csrc/jpeg.hip"

#include <cstdio>
#include <cstdlib>
#include <new>

namespace siftmi {
hipError_t host_wait_event(hipEvent_t) { return hipSuccess; }  // jpeg_decode_batch's; not called here
}  // namespace siftmi

using namespace siftmi;

static int decode(const uint8_t* d, size_t n, jpg::Header& H, jpg::Geom& g, std::vector<int16_t>& coef,
                  std::string& err) {
    int rc = jpg::parse(d, n, H, err);
    if (rc) return rc;
    g = jpg::geometry(H);
    if ((rc = jpg::check_support(H, g, err))) return rc;
    try {
        coef.assign(g.total * 64, 0);
    } catch (const std::bad_alloc&) {
        return err = "JPEG: host allocation failed", SIFT_MI_ENOMEM;
    }
    return jpg::entropy_decode(d, n, H, g, coef.data(), err);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    static char obuf[1 << 20];
    setvbuf(stdout, obuf, _IOFBF, sizeof obuf);
    for (int index = 0;; index++) {
        uint8_t lb[4];
        if (fread(lb, 1, 4, f) != 4) break;
        const size_t n = (size_t)lb[0] | (size_t)lb[1] << 8 | (size_t)lb[2] << 16 | (size_t)lb[3] << 24;
        uint8_t* d = (uint8_t*)malloc(n ? n : 1);
        if (!d || fread(d, 1, n, f) != n) return 3;
        if (!n) {  // a block of no bytes at all
            free(d);
            d = (uint8_t*)malloc(0);
        }
        auto* H = new jpg::Header;
        jpg::Geom g{};
        std::vector<int16_t> coef;
        std::string err;
        const int rc = decode(d, n, *H, g, coef, err);
        printf("stream %d %d %s\n", index, rc, err.c_str());
        if (rc == 0) {
            printf("frame %d %d %d %d %d %d %d\n", H->w, H->h, H->nc, g.hmax, g.vmax, g.mcux, g.mcuy);
            for (int k = 0; k < H->nc; k++) {
                const jpg::Comp& c = H->c[k];
                printf("comp %d %d %d %d %d %d %d %d %d\n", k, c.id, c.h, c.v, c.tq, c.td, c.ta, g.bw[k], g.bh[k]);
                printf("q %d", k);
                for (int i = 0; i < 64; i++) printf(" %d", H->q[c.tq][i]);
                printf("\ncoef %d", k);
                const int16_t* p = coef.data() + 64 * g.off[k];
                for (size_t i = 0; i < (size_t)g.bw[k] * g.bh[k] * 64; i++) printf(" %d", p[i]);
                printf("\n");
            }
        }
        delete H;
        free(d);
    }
    fclose(f);
    return 0;
}
