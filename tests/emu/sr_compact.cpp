// tests/emu/sr_compact.cpp — TEST HARNESS, NOT PRODUCT (part of tests/emu/libkernel_emu.so).  The program of hevc_amd/csrc/kernels/sr_compact.h (k_sr_compact)
// stepped on the CPU with the sequential executor, every workgroup of a launch, and the host side of hevc_amd/csrc/sr_compact_net.h (packing, launch list,
// memory).  As in sr.cpp: SeqExec::mfma_phase works the products out from the documented lane maps, every tensor a launch reads or writes is a copy allocated
// to its exact size (tests/test_sr_compact_cpu.py builds an AddressSanitizer program from this file, sr.cpp and tests/sr_compact_asan_main.cc), and a
// workgroup's LDS image starts as pseudo-random bytes.  `nwg` below the kernel's own count makes workgroups walk several tiles with few tiles.
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../hevc_amd/csrc/sr_compact_net.h"

using namespace mihevc;

extern "C" int emu_sr_input(const mihevc_rgb_format *fmt, int scale, int sw, int sh, const void *p0, const void *p1, const void *p2, int align, uint16_t *out, int order);

namespace {

// n bytes at a 16-byte boundary that end where the data ends
struct Exact {
    void *p = nullptr;
    size_t n = 0;
    Exact() = default;
    Exact(const Exact &) = delete;
    ~Exact() { free(p); }
    bool take(const void *src, size_t bytes)
    {
        n = bytes;
        if (posix_memalign(&p, 16, bytes ? bytes : 16)) return false;
        if (src) memcpy(p, src, bytes);
        else memset(p, 0xA5, bytes);
        return true;
    }
};

unsigned long long g_rnd;
template <class S> void scramble(S &s)
{
    unsigned char *b = (unsigned char *)&s;
    for (size_t i = 0; i < sizeof(S); i++) { g_rnd ^= g_rnd << 13; g_rnd ^= g_rnd >> 7; g_rnd ^= g_rnd << 17; b[i] = (unsigned char)(g_rnd >> 32); }
}
template <int CIN, int NA, int TAIL> void run(const SrCompactArgs &a, int order, int nwg)
{
    SeqExec ex;
    ex.order = order;
    std::unique_ptr<SrCompactShared<CIN, NA>> sh(new SrCompactShared<CIN, NA>);
    if (nwg < 1) nwg = sr_compact_workgroups(a.w, a.h);
    for (int wg = 0; wg < nwg; wg++) {
        scramble(*sh);
        sr_compact_program<CIN, NA, TAIL>(ex, *sh, a, wg, nwg);
    }
    scramble(*sh);
    sr_compact_program<CIN, NA, TAIL>(ex, *sh, a, sr_compact_tiles(a.w, a.h), nwg);      // one past the last tile: must do nothing
}
// the instances the product has (device.hip launch_sr_compact)
int conv(const SrCompactArgs &a, int cin, int tail, int order, int nwg)
{
    if (tail == 4 && cin == 64) run<64, 3, 4>(a, order, nwg);
    else if (tail == 2 && cin == 64) run<64, 1, 2>(a, order, nwg);
    else if (tail) return -3;
    else if (cin == 32) run<32, 4, 0>(a, order, nwg);
    else if (cin == 64) run<64, 4, 0>(a, order, nwg);
    else return -3;
    return 0;
}

}  // namespace

extern "C" {

// the tile in pixels, the rows of a wave, the most workgroups of a launch
void emu_sr_compact_tile(int *tw, int *th, int *rows, int *max_wg) { *tw = SRC_TW; *th = SRC_TH; *rows = SRC_ROWS; *max_wg = SRC_MAX_WG; }

// the flat weight count of a network, the device bytes of a source size, the number of launches and the arena's buffer offsets (X, A, B, OUT)
int emu_sr_compact_info(int scale, int convs, int sw, int sh, unsigned long long *count, unsigned long long *bytes, int *launches, unsigned long long *off4)
{
    const mihevc_sr_compact m = {scale, convs, {0, 0, 0, 0, 0, 0}};
    if (!sr_compact_ok(&m)) return -3;
    *count = sr_compact_count(scale, convs);
    *bytes = sr_compact_geometry_ok(sw, sh) ? sr_compact_bytes(scale, sw, sh) : 0;
    *launches = sr_compact_launches(convs);
    size_t off[SRC_BUFS];
    sr_compact_arena_layout(scale, sw, sh, off);
    for (int b = 0; b < SRC_BUFS; b++) off4[b] = off[b];
    return 0;
}
// the launch list as sr_compact_build makes it: per launch (layer, in_buf, out_buf, tail, cin_pad, cout_pad); `n`: the room in `out`, in launches.  Returns the count
int emu_sr_compact_launch_list(int scale, int convs, const float *weights, size_t count, int *out, int n)
{
    SrCompactNet net;
    if (!sr_compact_build(scale, convs, weights, count, net)) return -3;
    for (size_t i = 0; i < net.launches.size() && (int)i < n; i++) {
        const SrCompactLaunch &l = net.launches[i];
        const int v[6] = {l.layer, l.in_buf, l.out_buf, l.tail, net.layers[(size_t)l.layer].cin_pad, net.layers[(size_t)l.layer].cout_pad};
        memcpy(out + 6 * i, v, sizeof v);
    }
    return (int)net.launches.size();
}

// one launch: the arguments of mihevc_k_sr_compact_conv, then the SeqExec thread order, the seed of the LDS images and the number of workgroups (0: the
// kernel's own).  Returns 0, or -3
int emu_sr_compact_conv(const mihevc_sr_compact_conv_desc *d, const uint16_t *in, const float *weights, const float *bias, const float *slopes, const uint16_t *base,
                        uint16_t *out, int order, unsigned lds_seed, int nwg)
{
    if (!d || !in || !weights || !bias || !out || (d->cin != 32 && d->cin != 64) || d->cin_real < 1 || d->cin_real > d->cin) return -3;
    if (d->tail ? !base || d->cin != 64 || (d->scale != 2 && d->scale != 4) : !slopes) return -3;
    const int tail = d->tail ? d->scale : 0, cout = tail ? 3 * tail * tail : 64, cout_pad = (cout + SR_M - 1) / SR_M * SR_M;
    const size_t px = (size_t)d->width * d->height, out_n = px * (tail ? 3 * tail * tail : 64);
    std::vector<uint16_t> wpk(sr_packed_halves(cout_pad, d->cin));
    std::vector<float> b((size_t)cout_pad, 0.0f);
    sr_pack_layer(weights, cout, d->cin_real, cout_pad, d->cin, wpk.data());
    for (int c = 0; c < cout; c++) b[(size_t)c] = bias[c];
    Exact ein, ew, eb, es, ebase, eout;
    if (!ein.take(in, px * d->cin * 2) || !ew.take(wpk.data(), wpk.size() * 2) || !eb.take(b.data(), b.size() * 4) || !eout.take(out, out_n * 2)) return -5;
    if (!es.take(tail ? nullptr : slopes, tail ? 0 : 64 * 4) || !ebase.take(tail ? base : nullptr, tail ? px * SR_CIN0 * 2 : 0)) return -5;
    SrCompactArgs a;
    a.in = (const uint16_t *)ein.p; a.out = (uint16_t *)eout.p; a.wpk = (const uint16_t *)ew.p; a.bias = (const float *)eb.p; a.slope = (const float *)es.p;
    a.base = (const uint16_t *)ebase.p; a.w = d->width; a.h = d->height;
    g_rnd = 0x9E3779B97F4A7C15ull ^ lds_seed;
    if (int e = conv(a, d->cin, tail, order, nwg)) return e;
    memcpy(out, eout.p, out_n * 2);
    return 0;
}

// the whole network as mihevc_k_sr_compact_network runs it: k_sr_input, then every launch of the list over an arena of exactly sr_compact_bytes
int emu_sr_compact_network(const mihevc_sr_compact *model, const float *weights, size_t count, const mihevc_rgb_format *fmt, int sw, int sh, const void *p0,
                           const void *p1, const void *p2, uint16_t *out, int order, unsigned lds_seed)
{
    if (!sr_compact_ok(model) || !sr_compact_geometry_ok(sw, sh) || !out) return -3;
    SrCompactNet net;
    if (!sr_compact_build(model->scale, model->convs, weights, count, net)) return -3;
    size_t off[SRC_BUFS];
    Exact arena, x;
    if (!arena.take(nullptr, sr_compact_arena_layout(model->scale, sw, sh, off)) || arena.n != sr_compact_bytes(model->scale, sw, sh)) return -5;
    if (!x.take(nullptr, (size_t)sw * sh * SR_CIN0 * 2)) return -5;
    if (int e = emu_sr_input(fmt, 4, sw, sh, p0, p1, p2, 16, (uint16_t *)x.p, order)) return e;      // (odd sides: the kernel runs as for scale 4)
    memcpy((uint8_t *)arena.p + off[SRC_X], x.p, x.n);
    g_rnd = 0x9E3779B97F4A7C15ull ^ lds_seed;
    if (int e = sr_compact_for_each_launch(net, (uint8_t *)arena.p, net.wpk.data(), net.par.data(), sw, sh,
                                           [&](int cin, int tail, const SrCompactArgs &a) { return conv(a, cin, tail, order, 0); })) return e;
    memcpy(out, (uint8_t *)arena.p + off[SRC_OUT], (size_t)sw * sh * model->scale * model->scale * 3 * 2);
    return 0;
}

}  // extern "C"
