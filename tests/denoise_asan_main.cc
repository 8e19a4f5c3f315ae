// tests/denoise_asan_main.cc — TEST HARNESS, NOT PRODUCT.  A stand-alone program over tests/emu/denoise.cpp for an AddressSanitizer / UBSan build
// (tests/test_denoise_cpu.py compiles the two files with -fsanitize=address,undefined and runs the result): the stepped k_denoise over source planes that end
// with the last sample of their last row, every size of the tests, both element types, every alignment class, four strengths.  A read past a source plane, a write
// past an output plane or the LDS images, or a signed overflow ends the program with the sanitizer's report; exit status 0 otherwise.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/mihevc.h"

extern "C" int emu_denoise(const mihevc_denoise *dn, const void *const *prev, const void *const *cur, const void *const *next, int w, int h, int depth, int order, int align,
                           unsigned lds_seed, void *out_y, void *out_u, void *out_v, int *stats);

int main()
{
    const int sizes[][2] = {{16, 16}, {70, 36}, {264, 72}, {136, 20}, {130, 66}};
    const int aligns[4] = {16, 8, 4, 1};
    const mihevc_denoise strengths[4] = {{0, 0, 0, 0, {0, 0, 0, 0}}, {255, 255, 255, 255, {0, 0, 0, 0}}, {12, 0, 0, 16, {0, 0, 0, 0}}, {5, 7, 5, 7, {0, 0, 0, 0}}};
    uint32_t rnd = 2463534242u;
    int runs = 0;
    for (auto &sz : sizes)
        for (int depth : {8, 10})
            for (int align : aligns)
                for (auto &dn : strengths) {
                    const int w = sz[0], h = sz[1], es = depth > 8 ? 2 : 1, pw = (w + 7) & ~7, ph = (h + 7) & ~7;
                    std::vector<uint8_t> planes[9];
                    const void *p[3][3];
                    for (int f = 0; f < 3; f++)
                        for (int c = 0; c < 3; c++) {
                            auto &v = planes[3 * f + c];
                            v.resize((size_t)(c ? w * h / 4 : w * h) * es);
                            for (auto &b : v) { rnd = rnd * 1664525u + 1013904223u; b = (uint8_t)(rnd >> 24); }      // 16-bit elements: values above the depth too
                            p[f][c] = v.data();
                        }
                    std::vector<uint8_t> oy((size_t)pw * ph * es), ou((size_t)pw * ph / 4 * es), ov(ou.size());
                    int stats[4] = {0, 0, 0, 0};
                    const int rc = emu_denoise(&dn, p[0], p[1], p[2], w, h, depth, runs % 3, align, (unsigned)runs, oy.data(), ou.data(), ov.data(), stats);
                    if (rc || stats[0] || stats[1] || stats[2] != align || stats[3] != align) {
                        fprintf(stderr, "%dx%d depth %d align %d strengths %d %d %d %d: rc %d, misaligned %d, spilled %d, planes of class %d / %d\n", w, h, depth, align,
                                dn.luma_spatial, dn.luma_temporal, dn.chroma_spatial, dn.chroma_temporal, rc, stats[0], stats[1], stats[2], stats[3]);
                        return 1;
                    }
                    runs++;
                }
    printf("%d runs\n", runs);
    return 0;
}
