// tests/ingest_asan_main.cc — TEST HARNESS, NOT PRODUCT.  A stand-alone program over tests/emu/ingest.cpp for an AddressSanitizer / UBSan build
// (tests/test_ingest_cpu.py compiles the two files with -fsanitize=address,undefined and runs the result): the stepped k_ingest over source planes that end
// with the last sample of their last row, every layout, element type and alignment class, at sizes with and without a margin.  A read past a source plane or a
// write past an output plane ends the program with the sanitizer's report; exit status 0 otherwise.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/mihevc.h"

extern "C" int emu_ingest(const mihevc_src_format *fmt, const void *y, const void *u, const void *v, int w, int h, int out_depth, int order, int align, void *out_y,
                          void *out_u, void *out_v, int *stats);

int main()
{
    const int sizes[3][2] = {{16, 16}, {72, 40}, {70, 38}}, aligns[4] = {16, 8, 4, 1}, depths[3] = {8, 10, 16};
    uint32_t rnd = 12345;
    int runs = 0;
    for (int chroma : {420, 422, 444})
        for (int semi = 0; semi < 2; semi++)
            for (int bits : depths)
                for (int msb = 0; msb <= (bits > 8 ? 1 : 0); msb++)
                    for (auto &sz : sizes)
                        for (int align : aligns)
                            for (int out_depth : {8, 10}) {
                                const mihevc_src_format f = {chroma, semi, bits, msb, {0, 0, 0, 0}};
                                const int w = sz[0], h = sz[1], es = bits > 8 ? 2 : 1, pw = (w + 7) & ~7, ph = (h + 7) & ~7;
                                const int crow = (chroma == 444 ? w : w / 2) * (semi ? 2 : 1), crows = chroma == 420 ? h / 2 : h;
                                std::vector<uint8_t> y((size_t)w * h * es), u((size_t)crow * crows * es), v(semi ? 0 : u.size());
                                for (auto *p : {&y, &u, &v})
                                    for (auto &b : *p) { rnd = rnd * 1664525u + 1013904223u; b = (uint8_t)(rnd >> 24); }
                                const size_t eo = out_depth > 8 ? 2 : 1;
                                std::vector<uint8_t> oy((size_t)pw * ph * eo), ou((size_t)pw * ph / 4 * eo), ov(ou.size());
                                int stats[4] = {0, 0, 0, 0};
                                const int rc = emu_ingest(&f, y.data(), u.data(), semi ? nullptr : v.data(), w, h, out_depth, runs % 3, align, oy.data(), ou.data(), ov.data(), stats);
                                if (rc || stats[0] || stats[1] || stats[2] != align || stats[3] != align) {
                                    fprintf(stderr, "chroma %d semi %d bits %d msb %d %dx%d align %d -> %d: rc %d, misaligned %d, spilled %d, ran with %d / %d\n", chroma, semi, bits, msb, w, h,
                                            align, out_depth, rc, stats[0], stats[1], stats[2], stats[3]);
                                    return 1;
                                }
                                runs++;
                            }
    printf("%d runs\n", runs);
    return 0;
}
