// tests/lut3d_asan_main.cc — TEST HARNESS, NOT PRODUCT.  A stand-alone program over tests/emu/lut3d.cpp for an AddressSanitizer / UBSan build
// (tests/test_lut3d_cpu.py compiles the two files with -fsanitize=address,undefined and runs the result): the stepped k_lut3d over source planes that end with the
// last sample of their last row and a packed table that ends with its last entry, every size of the tests, the three source depths, both output depths, every
// alignment class, four table sizes; then the division check.  A read past a source plane or the table, a write past an output plane, or a signed overflow ends the
// program with the sanitizer's report; exit status 0 otherwise.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/mihevc.h"

extern "C" int emu_lut3d(const mihevc_lut3d_src *src, int n, const uint16_t *table, const void *y, const void *u, const void *v, int w, int h, int out_depth,
                         int out_matrix, int out_full, int order, int align, void *out_y, void *out_u, void *out_v, int *stats);
extern "C" int emu_lut3d_div_check();

int main()
{
    const int sizes[][2] = {{16, 16}, {70, 36}, {520, 72}, {136, 20}};
    const int aligns[4] = {16, 8, 4, 1}, ns[4] = {2, 17, 33, 65}, matrices[4] = {1, 5, 6, 9};
    uint32_t rnd = 2463534242u;
    int runs = 0;
    for (auto &sz : sizes)
        for (int bits : {8, 10, 12})
            for (int depth : {8, 10})
                for (int align : aligns) {
                    const int w = sz[0], h = sz[1], es = bits > 8 ? 2 : 1, os = depth > 8 ? 2 : 1, pw = (w + 7) & ~7, ph = (h + 7) & ~7, n = ns[runs % 4];
                    std::vector<uint8_t> planes[3];
                    for (int c = 0; c < 3; c++) {
                        planes[c].resize((size_t)(c ? w * h / 4 : w * h) * es);
                        for (auto &b : planes[c]) { rnd = rnd * 1664525u + 1013904223u; b = (uint8_t)(rnd >> 24); }      // 16-bit elements: values above the depth too
                    }
                    std::vector<uint16_t> table((size_t)n * n * n * 3);
                    for (auto &t : table) { rnd = rnd * 1664525u + 1013904223u; t = (uint16_t)(rnd >> 16); }
                    table[0] = 0; table[1] = 65535; table[table.size() - 1] = 65535;
                    std::vector<uint8_t> oy((size_t)pw * ph * os), ou((size_t)pw * ph / 4 * os), ov(ou.size());
                    const mihevc_lut3d_src src = {bits, matrices[runs % 4], (runs / 4) % 2, {0, 0, 0, 0}};
                    int stats[4] = {0, 0, 0, 0};
                    const int rc = emu_lut3d(&src, n, table.data(), planes[0].data(), planes[1].data(), planes[2].data(), w, h, depth, matrices[(runs / 2) % 4], (runs / 3) % 2,
                                             runs % 3, align, oy.data(), ou.data(), ov.data(), stats);
                    if (rc || stats[0] || stats[1] || stats[2] != align || stats[3] != align) {
                        fprintf(stderr, "%dx%d bits %d depth %d align %d n %d: rc %d, misaligned %d, spilled %d, planes of class %d / %d\n", w, h, bits, depth, align, n, rc,
                                stats[0], stats[1], stats[2], stats[3]);
                        return 1;
                    }
                    runs++;
                }
    if (int bad = emu_lut3d_div_check()) {
        fprintf(stderr, "%d wrong quotients\n", bad);
        return 1;
    }
    printf("%d runs\n", runs);
    return 0;
}
