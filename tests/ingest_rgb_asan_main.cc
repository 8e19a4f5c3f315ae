// tests/ingest_rgb_asan_main.cc — TEST HARNESS, NOT PRODUCT.  A stand-alone program over tests/emu/ingest_rgb.cpp for an AddressSanitizer / UBSan build
// (tests/test_ingest_rgb_cpu.py compiles the two files with -fsanitize=address,undefined and runs the result): the stepped k_ingest_rgb over source planes that
// end with the last sample of their last row, every layout, element type and alignment class, at sizes with and without a margin.  A read past a source plane
// or a write past an output plane ends the program with the sanitizer's report; exit status 0 otherwise.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/mihevc.h"

extern "C" int emu_ingest_rgb(const mihevc_rgb_format *fmt, const void *p0, const void *p1, const void *p2, int w, int h, int out_depth, int order, int align,
                              void *out_y, void *out_u, void *out_v, int *stats);

int main()
{
    const int sizes[3][2] = {{16, 16}, {72, 40}, {70, 38}}, aligns[4] = {16, 8, 4, 1}, matrices[4] = {1, 5, 6, 9};
    // layout, sample, bit depth
    const int kinds[8][3] = {{0, 0, 8}, {0, 0, 10}, {0, 0, 16}, {0, 1, 0}, {0, 2, 0}, {3, 0, 8}, {3, 0, 16}, {4, 0, 8}};
    uint32_t rnd = 12345;
    int runs = 0;
    for (auto &k : kinds)
        for (auto &sz : sizes)
            for (int align : aligns)
                for (int out_depth : {8, 10}) {
                    const int layout = k[0], n = layout ? layout : 3;
                    const mihevc_rgb_format f = {layout, (runs + 2) % n, (runs + 1) % n, runs % n, k[1], k[2], matrices[runs % 4], 1 + runs / 4 % 2, {0, 0, 0, 0}};
                    const int w = sz[0], h = sz[1], es = k[1] == 2 ? 4 : k[1] == 1 || k[2] > 8 ? 2 : 1, pw = (w + 7) & ~7, ph = (h + 7) & ~7;
                    std::vector<uint8_t> p[3];
                    for (int c = 0; c < (layout ? 1 : 3); c++) {
                        p[c].resize((size_t)w * h * (layout ? layout : 1) * es);
                        for (auto &b : p[c]) { rnd = rnd * 1664525u + 1013904223u; b = (uint8_t)(rnd >> 24); }      // floats: every bit pattern, NaN and infinities too
                    }
                    const size_t eo = out_depth > 8 ? 2 : 1;
                    std::vector<uint8_t> oy((size_t)pw * ph * eo), ou((size_t)pw * ph / 4 * eo), ov(ou.size());
                    int stats[4] = {0, 0, 0, 0};
                    const int rc = emu_ingest_rgb(&f, p[0].data(), layout ? nullptr : p[1].data(), layout ? nullptr : p[2].data(), w, h, out_depth, runs % 3, align, oy.data(),
                                                  ou.data(), ov.data(), stats);
                    const int want = align == 1 && es == 4 ? 4 : align;      // a float32 one element off is still 4-byte aligned
                    if (rc || stats[0] || stats[1] || stats[2] != want) {
                        fprintf(stderr, "layout %d sample %d bits %d %dx%d align %d -> %d: rc %d, misaligned %d, spilled %d, ran with %d\n", layout, k[1], k[2], w, h, align,
                                out_depth, rc, stats[0], stats[1], stats[2]);
                        return 1;
                    }
                    runs++;
                }
    printf("%d runs\n", runs);
    return 0;
}
