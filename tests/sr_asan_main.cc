// tests/sr_asan_main.cc — TEST HARNESS, NOT PRODUCT.  A stand-alone program over tests/emu/sr.cpp for an AddressSanitizer / UBSan build (tests/test_sr_cpu.py
// compiles the two files with -fsanitize=address,undefined and runs the result): the packer and the stepped k_sr_conv over tensors allocated to end with their
// last element, every channel shape of the network at sizes below, at and above a tile, with the folded enlargement, the planar output and both residuals; the
// stepped k_sr_input over planes that end with their last sample, every element type and alignment class; one whole network over an arena of exactly the stated
// size.  A read or write past a tensor, a plane, the arena or the LDS image, or a signed overflow, ends the program with the sanitizer's report.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/mihevc.h"

extern "C" int emu_sr_conv(const mihevc_sr_conv_desc *d, const uint16_t *in, const float *weights, const float *bias, const uint16_t *r1, const uint16_t *r2,
                           uint16_t *out, int order, unsigned lds_seed);
extern "C" int emu_sr_input(const mihevc_rgb_format *fmt, int scale, int sw, int sh, const void *p0, const void *p1, const void *p2, int align, uint16_t *out, int order);
extern "C" int emu_sr_network(const mihevc_sr_model *model, const float *weights, size_t count, const mihevc_rgb_format *fmt, int sw, int sh, const void *p0,
                              const void *p1, const void *p2, uint16_t *out, int order, unsigned lds_seed);
extern "C" int emu_sr_net_info(int scale, int blocks, int sw, int sh, unsigned long long *count, unsigned long long *bytes, int *launches);

int main()
{
    // cin, cin_real, in_ch, cout, out_ch, out_off, planar
    const int shapes[][7] = {{32, 3, 32, 64, 64, 0, 0},      {32, 12, 32, 64, 192, 0, 0},   {64, 64, 192, 32, 192, 64, 0}, {96, 96, 192, 32, 192, 96, 0},
                             {128, 128, 192, 32, 192, 128, 0}, {160, 160, 192, 32, 192, 160, 0}, {192, 192, 192, 64, 192, 0, 0}, {64, 64, 64, 64, 64, 0, 0},
                             {64, 64, 64, 3, 3, 0, 1}};
    const int sizes[][2] = {{4, 4}, {15, 7}, {16, 8}, {17, 9}, {18, 8}, {10, 14}};
    const uint16_t vals[3] = {0xBC00, 0, 0x3C00};      // -1, 0, 1
    uint32_t rnd = 12345;
    auto next = [&]() { rnd = rnd * 1664525u + 1013904223u; return rnd >> 8; };
    int runs = 0;
    for (auto &sp : shapes)
        for (auto &sz : sizes)
            for (int up = 0; up < 2; up++) {
                const int w = sz[0], h = sz[1];
                if (up && ((w | h) & 1)) continue;
                const int sw = up ? w / 2 : w, sh = up ? h / 2 : h, n_res = sp[6] ? 0 : runs % 3;
                const mihevc_sr_conv_desc d = {w, h, up, sp[6], runs & 1, n_res, sp[2], 0, sp[0], sp[1], sp[4], sp[5], sp[3], 192, 0, 64, 0, 0.25f, 0.5f, 0.5f};
                std::vector<uint16_t> in((size_t)sw * sh * sp[2]), r1((size_t)w * h * 192), r2((size_t)w * h * 64), out((size_t)w * h * (sp[6] ? 3 : sp[4]));
                for (auto *t : {&in, &r1, &r2}) for (auto &v : *t) v = vals[next() % 3];
                std::vector<float> wt((size_t)sp[3] * sp[1] * 9), bias((size_t)sp[3]);
                for (auto &v : wt) v = (float)(int)(next() % 3) - 1.0f;
                for (auto &v : bias) v = (float)(int)(next() % 64);
                const int rc = emu_sr_conv(&d, in.data(), wt.data(), bias.data(), r1.data(), r2.data(), out.data(), runs % 3, (unsigned)runs);
                if (rc) { fprintf(stderr, "conv %d -> %d at %dx%d up %d: rc %d\n", sp[0], sp[3], w, h, up, rc); return 1; }
                runs++;
            }
    // the input kernel: planes, packed 3 and 4, 8 and 16 bit, half and single floats; every alignment class; both scales
    const mihevc_rgb_format fmts[] = {{0, 2, 0, 1, 0, 8, 0, 0, {0, 0, 0, 0}},  {3, 0, 1, 2, 0, 8, 0, 0, {0, 0, 0, 0}},  {4, 2, 1, 0, 0, 8, 0, 0, {0, 0, 0, 0}},
                                      {0, 2, 0, 1, 0, 10, 0, 0, {0, 0, 0, 0}}, {3, 0, 1, 2, 0, 16, 0, 0, {0, 0, 0, 0}}, {0, 2, 0, 1, 1, 0, 0, 0, {0, 0, 0, 0}},
                                      {0, 2, 0, 1, 2, 0, 0, 0, {0, 0, 0, 0}}};
    for (auto &f : fmts)
        for (int align : {16, 8, 4, 1})
            for (int scale : {4, 2}) {
                const int sw = 22, sh = 14, es = f.sample == 2 ? 4 : f.sample == 1 || f.bit_depth > 8 ? 2 : 1, row = (f.layout ? f.layout : 1) * sw;
                if (align < es && align != 1) continue;
                std::vector<uint8_t> p[3];
                for (auto &v : p) { v.resize((size_t)row * sh * es); for (auto &b : v) b = (uint8_t)next(); }
                std::vector<uint16_t> out((size_t)sw * sh * 32);
                const int rc = emu_sr_input(&f, scale, sw, sh, p[0].data(), p[1].data(), p[2].data(), align, out.data(), runs % 3);
                if (rc) { fprintf(stderr, "input layout %d sample %d depth %d align %d scale %d: rc %d\n", f.layout, f.sample, f.bit_depth, align, scale, rc); return 1; }
                runs++;
            }
    // one network of each scale, small: the arena is exactly sr_net_bytes
    for (int scale : {4, 2}) {
        unsigned long long count = 0, bytes = 0;
        int launches = 0;
        if (emu_sr_net_info(scale, 1, 6, 10, &count, &bytes, &launches) || !bytes) return 1;
        std::vector<float> w((size_t)count);
        for (auto &v : w) v = ((float)(int)(next() % 2001) - 1000.0f) * 2e-5f;
        std::vector<uint8_t> p[3];
        for (auto &v : p) { v.resize(60); for (auto &b : v) b = (uint8_t)next(); }
        std::vector<uint16_t> out((size_t)3 * 60 * scale * scale);
        const mihevc_sr_model m = {scale, 1, {0, 0, 0, 0, 0, 0}};
        const int rc = emu_sr_network(&m, w.data(), (size_t)count, &fmts[0], 6, 10, p[0].data(), p[1].data(), p[2].data(), out.data(), 2, 99u);
        if (rc) { fprintf(stderr, "network x%d: rc %d\n", scale, rc); return 1; }
        runs++;
    }
    printf("%d runs\n", runs);
    return 0;
}
