// tests/emu/sr_yuv.cpp — TEST HARNESS, NOT PRODUCT (part of tests/emu/libkernel_emu.so).  The program of hevc_amd/csrc/kernels/sr_yuv.h (k_sr_from_yuv) stepped on
// the CPU with the sequential executor, every workgroup of the launch and one past the last, and the network behind it as tests/emu/sr.cpp runs it.  The source
// planes keep the caller's pitches, start at a 64-byte boundary or one element behind one, and end with the last sample of their last row; the tensor and the
// arena are allocated to their exact size (a read or write past any of them is a finding of the AddressSanitizer program tests/test_sr_yuv_cpu.py builds from
// this file and tests/sr_yuv_asan_main.cc, which is why this file stands alone and repeats the few lines of sr.cpp that choose an instance of k_sr_conv).  The
// kernel has no LDS.  hevc_amd/ never loads this library.
#include <cstdlib>
#include <cstring>
#include <memory>

#include "ingest_planes.h"
#include "../../hevc_amd/csrc/kernels/sr_yuv.h"
#include "../../hevc_amd/csrc/sr_net.h"

using namespace mihevc;

namespace {

// n bytes at a 16-byte boundary that end where the data ends
struct Exact {
    void *p = nullptr;
    size_t n = 0;
    Exact() = default;
    Exact(const Exact &) = delete;
    ~Exact() { free(p); }
    bool take(size_t bytes)
    {
        n = bytes;
        if (posix_memalign(&p, 16, bytes ? bytes : 16)) return false;
        memset(p, 0xA5, bytes);
        return true;
    }
};
// a source plane as the caller laid it out: `row` elements in each of `rows` rows `pitch` apart, copied to an allocation that ends with the last sample;
// off_one: the plane starts one element behind a 64-byte boundary
template <typename TI> struct Placed {
    void *base = nullptr;
    const TI *p = nullptr;
    Placed() = default;
    Placed(const Placed &) = delete;
    ~Placed() { free(base); }
    bool place(const void *src, int row, int rows, int pitch, bool off_one)
    {
        const size_t off = off_one ? sizeof(TI) : 0, bytes = ((size_t)pitch * (rows - 1) + row) * sizeof(TI);
        if (posix_memalign(&base, 64, off + bytes)) return false;
        memset(base, 0x5A, off);
        memcpy((uint8_t *)base + off, src, bytes);
        p = (const TI *)((uint8_t *)base + off);
        return true;
    }
};

template <typename TI> int from_yuv(const mihevc_sr_yuv &f, int scale, const void *const *src, int pitch_y, int pitch_c, bool off_one, uint16_t *out, int order)
{
    Placed<TI> sp[3];
    for (int c = 0; c < 3; c++)
        if (!sp[c].place(src[c], c ? f.width / 2 : f.width, c ? f.height / 2 : f.height, c ? pitch_c : pitch_y, off_one)) return -5;
    const SrYuvArgs a = sr_yuv_args(f, scale, sp[0].p, sp[1].p, sp[2].p, pitch_y, pitch_c, out);
    SeqExec ex;
    ex.order = order;
    g_ingest_misaligned = 0;
    const int nwg = sr_yuv_workgroups(f.width, f.height);
    for (int wg = 0; wg <= nwg; wg++) sr_from_yuv_program<TI>(ex, a, wg);      // one past the last: must do nothing
    return g_ingest_misaligned ? -6 : 0;
}
int from_yuv_any(const mihevc_sr_yuv &f, int scale, const void *const *src, int pitch_y, int pitch_c, bool off_one, uint16_t *out, int order)
{
    if (f.bit_depth > 8) return from_yuv<uint16_t>(f, scale, src, pitch_y, pitch_c, off_one, out, order);
    return from_yuv<uint8_t>(f, scale, src, pitch_y, pitch_c, off_one, out, order);
}
bool args_ok(const mihevc_sr_yuv *f, int scale, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, const void *out)
{
    return sr_yuv_src_ok(f) && (scale == 2 || scale == 4) && out && sr_yuv_planes_ok(*f, y, u, v, pitch_y, pitch_c);
}

unsigned long long g_lds_rnd;
template <class S> void scramble(S &s)
{
    unsigned char *b = (unsigned char *)&s;
    for (size_t i = 0; i < sizeof(S); i++) { g_lds_rnd ^= g_lds_rnd << 13; g_lds_rnd ^= g_lds_rnd >> 7; g_lds_rnd ^= g_lds_rnd << 17; b[i] = (unsigned char)(g_lds_rnd >> 32); }
}
template <int CIN, int NB, bool PLANAR> void run_conv(const SrConvArgs &a, int order)
{
    SeqExec ex;
    ex.order = order;
    std::unique_ptr<SrShared<CIN>> sh(new SrShared<CIN>);
    const int nwg = sr_conv_workgroups(a.w, a.h);
    for (int wg = 0; wg <= nwg; wg++) {
        scramble(*sh);
        sr_conv_program<CIN, NB, PLANAR>(ex, *sh, a, wg);
    }
}
// the instances the product has (device.hip launch_sr_conv), as tests/emu/sr.cpp chooses them
int conv(const SrConvArgs &a, int cin, int cout, bool planar, int order)
{
    if (planar && cin == 64 && cout == 16) run_conv<64, 1, true>(a, order);
    else if (planar) return -3;
    else if (cin == 32 && cout == 64) run_conv<32, 4, false>(a, order);
    else if (cin == 64 && cout == 64) run_conv<64, 4, false>(a, order);
    else if (cin == 192 && cout == 64) run_conv<192, 4, false>(a, order);
    else if (cin == 64 && cout == 32) run_conv<64, 2, false>(a, order);
    else if (cin == 96 && cout == 32) run_conv<96, 2, false>(a, order);
    else if (cin == 128 && cout == 32) run_conv<128, 2, false>(a, order);
    else if (cin == 160 && cout == 32) run_conv<160, 2, false>(a, order);
    else return -3;
    return 0;
}

}  // namespace

extern "C" {

// k_sr_from_yuv: the arguments of mihevc_k_sr_from_yuv, then off_one (the planes start one element behind an aligned address) and the SeqExec thread order.
// out: the tensor, (W x H or W/2 x H/2) x 32 halves.  Returns 0, -3 for what the stage entry refuses, -6 for an access that is not aligned to its width
int emu_sr_from_yuv(const mihevc_sr_yuv *src, int scale, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, uint16_t *out, int off_one, int order)
{
    if (!args_ok(src, scale, y, u, v, pitch_y, pitch_c, out)) return -3;
    Exact eo;
    const size_t n = (size_t)src->width * src->height * SR_CIN0 * 2 / (scale == 2 ? 4 : 1);
    if (!eo.take(n)) return -5;
    const void *p[3] = {y, u, v};
    if (int e = from_yuv_any(*src, scale, p, pitch_y, pitch_c, off_one != 0, (uint16_t *)eo.p, order)) return e;
    memcpy(out, eo.p, n);
    return 0;
}

// the whole network over a Y'CbCr source: k_sr_from_yuv, then every launch emu_sr_network runs, over an arena of exactly sr_net_bytes.  out: three planes of
// halves, scale x the source size
int emu_sr_network_yuv(const mihevc_sr_model *model, const float *weights, size_t count, const mihevc_sr_yuv *src, const void *y, const void *u, const void *v,
                       int pitch_y, int pitch_c, uint16_t *out, int order, unsigned lds_seed)
{
    if (!sr_model_ok(model) || !weights || !args_ok(src, model->scale, y, u, v, pitch_y, pitch_c, out)) return -3;
    SrNet net;
    if (!sr_net_build(model->scale, model->blocks, weights, count, net)) return -3;
    const int f = model->scale == 2 ? 2 : 1, tw = src->width / f, th = src->height / f;
    size_t off[SR_BUFS];
    Exact arena;
    if (!arena.take(sr_arena_layout(tw, th, off)) || arena.n != sr_net_bytes(model->scale, src->width, src->height)) return -5;
    const void *p[3] = {y, u, v};
    if (int e = from_yuv_any(*src, model->scale, p, pitch_y, pitch_c, false, (uint16_t *)((uint8_t *)arena.p + off[SR_X]), order)) return e;
    g_lds_rnd = 0x9E3779B97F4A7C15ull ^ lds_seed;
    if (int e = sr_for_each_launch(net, (uint8_t *)arena.p, net.wpk.data(), net.bias.data(), tw, th,
                                   [&](int cin, int cout, bool planar, const SrConvArgs &a) { return conv(a, cin, cout, planar, order); })) return e;
    memcpy(out, (uint8_t *)arena.p + off[SR_OUT], (size_t)tw * th * 16 * 3 * 2);
    return 0;
}

}  // extern "C"
