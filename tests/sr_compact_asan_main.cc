// tests/sr_compact_asan_main.cc — TEST HARNESS, NOT PRODUCT.  A stand-alone program over tests/emu/sr_compact.cpp (with tests/emu/sr.cpp for the input kernel)
// for an AddressSanitizer / UBSan build (tests/test_sr_compact_cpu.py compiles the files with -fsanitize=address,undefined and runs the result): the packer
// and the stepped k_sr_compact over tensors allocated to end with their last element, every instance at sizes below, at and above a tile, with the kernel's own
// number of workgroups and with fewer; one whole network of each scale, an odd size included, over an arena of exactly the stated size.  A read or write
// past a tensor, the arena or the LDS image, or a signed overflow, ends the program with the sanitizer's report.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/mihevc.h"

extern "C" int emu_sr_compact_conv(const mihevc_sr_compact_conv_desc *d, const uint16_t *in, const float *weights, const float *bias, const float *slopes,
                                   const uint16_t *base, uint16_t *out, int order, unsigned lds_seed, int nwg);
extern "C" int emu_sr_compact_network(const mihevc_sr_compact *model, const float *weights, size_t count, const mihevc_rgb_format *fmt, int sw, int sh,
                                      const void *p0, const void *p1, const void *p2, uint16_t *out, int order, unsigned lds_seed);
extern "C" int emu_sr_compact_info(int scale, int convs, int sw, int sh, unsigned long long *count, unsigned long long *bytes, int *launches, unsigned long long *off4);

int main()
{
    // cin, cin_real, tail, scale
    const int shapes[][4] = {{32, 3, 0, 0}, {64, 64, 0, 0}, {64, 64, 1, 4}, {64, 64, 1, 2}};
    const int sizes[][2] = {{4, 4}, {15, 15}, {16, 16}, {17, 17}, {33, 18}, {5, 35}};
    const uint16_t vals[3] = {0xBC00, 0, 0x3C00};      // -1, 0, 1
    uint32_t rnd = 12345;
    auto next = [&]() { rnd = rnd * 1664525u + 1013904223u; return rnd >> 8; };
    int runs = 0;
    for (auto &sp : shapes)
        for (auto &sz : sizes)
            for (int nwg : {0, 2}) {
                const int w = sz[0], h = sz[1], r = sp[3], cout = sp[2] ? 3 * r * r : 64;
                const mihevc_sr_compact_conv_desc d = {w, h, sp[0], sp[1], sp[2], sp[3], {0, 0}};
                std::vector<uint16_t> in((size_t)w * h * sp[0]), base((size_t)w * h * 32), out((size_t)w * h * cout);
                for (auto *t : {&in, &base}) for (auto &v : *t) v = vals[next() % 3];
                std::vector<float> wt((size_t)cout * sp[1] * 9), bias((size_t)cout), slopes(64);
                for (auto &v : wt) v = (float)(int)(next() % 3) - 1.0f;
                for (auto &v : bias) v = (float)(int)(next() % 64);
                for (auto &v : slopes) v = 0.25f * (float)(int)(next() % 5) - 0.5f;
                const int rc = emu_sr_compact_conv(&d, in.data(), wt.data(), bias.data(), sp[2] ? nullptr : slopes.data(), sp[2] ? base.data() : nullptr, out.data(),
                                                   runs % 3, (unsigned)runs, nwg);
                if (rc) { fprintf(stderr, "conv %d tail %d x%d at %dx%d: rc %d\n", sp[0], sp[2], sp[3], w, h, rc); return 1; }
                runs++;
            }
    const mihevc_rgb_format gbrp = {0, 2, 0, 1, 0, 8, 0, 0, {0, 0, 0, 0}};
    const int nets[][3] = {{4, 6, 10}, {2, 6, 10}, {2, 7, 19}};      // scale, source size
    for (auto &n : nets) {
        unsigned long long count = 0, bytes = 0, off[4];
        int launches = 0;
        if (emu_sr_compact_info(n[0], 2, n[1], n[2], &count, &bytes, &launches, off) || !bytes || launches != 4) return 1;
        std::vector<float> w((size_t)count);
        for (auto &v : w) v = ((float)(int)(next() % 2001) - 1000.0f) * 5e-5f;
        std::vector<uint8_t> p[3];
        for (auto &v : p) { v.resize((size_t)n[1] * n[2]); for (auto &b : v) b = (uint8_t)next(); }
        std::vector<uint16_t> out((size_t)3 * n[1] * n[2] * n[0] * n[0]);
        const mihevc_sr_compact m = {n[0], 2, {0, 0, 0, 0, 0, 0}};
        const int rc = emu_sr_compact_network(&m, w.data(), (size_t)count, &gbrp, n[1], n[2], p[0].data(), p[1].data(), p[2].data(), out.data(), 2, 99u);
        if (rc) { fprintf(stderr, "network x%d %dx%d: rc %d\n", n[0], n[1], n[2], rc); return 1; }
        runs++;
    }
    printf("%d runs\n", runs);
    return 0;
}
