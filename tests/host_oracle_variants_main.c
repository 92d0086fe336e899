/* The CPU oracle under AddressSanitizer and UBSan, as a stand-alone program
 * (tests/test_refine_variants_cpu.py builds it together with
 * oracle/sift_oracle.c and runs it): every wrong-on-purpose variant of the
 * refinement and orientation decisions, each on its own, over raw u8 frames.
 * A variant that read outside the planes would stop the program here.
 *
 *   host_oracle_variants W H FILE [W H FILE ...]
 * prints one line per (file, profile, variant bit): "n FILE PROFILE BIT COUNT".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

void oracle_set_variant(int64_t v);
void* oracle_sift(const uint8_t* img, int w, int h, int stride, int profile, int64_t features_limit);
size_t oracle_result_n(const void* r);
void oracle_result_free(void* r);

int main(int argc, char** argv) {
    if (argc < 4 || (argc - 1) % 3 != 0) {
        fprintf(stderr, "usage: %s W H FILE [W H FILE ...]\n", argv[0]);
        return 2;
    }
    for (int a = 1; a + 2 < argc; a += 3) {
        const int w = atoi(argv[a]), h = atoi(argv[a + 1]);
        if (w < 1 || h < 1 || w > 4096 || h > 4096) return 2;
        const size_t n = (size_t)w * h;
        uint8_t* img = (uint8_t*)malloc(n);
        FILE* f = fopen(argv[a + 2], "rb");
        if (!img || !f || fread(img, 1, n, f) != n) {
            fprintf(stderr, "cannot read %s\n", argv[a + 2]);
            return 2;
        }
        fclose(f);
        for (int profile = 0; profile < 2; profile++)
            for (int bit = -1; bit < 32; bit++) {
                if (bit >= 0 && bit < 16) continue; /* the variants of this test: none, then bits 16..31 */
                oracle_set_variant(bit < 0 ? 0 : (int64_t)1 << bit);
                void* r = oracle_sift(img, w, h, w, profile, -1);
                if (!r) return 3;
                printf("n %s %d %d %zu\n", argv[a + 2], profile, bit, oracle_result_n(r));
                oracle_result_free(r);
            }
        oracle_set_variant(0);
        free(img);
    }
    return 0;
}
