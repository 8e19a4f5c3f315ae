// tests/emu/sr.cpp — TEST HARNESS, NOT PRODUCT (part of tests/emu/libkernel_emu.so).  The programs of hevc_amd/csrc/kernels/sr_conv.h (k_sr_conv, k_sr_input)
// stepped on the CPU with the sequential executor, every workgroup of a launch, and the host side of hevc_amd/csrc/sr_net.h (packing, launch list, memory).
// SeqExec::mfma_phase works the matrix products out from the documented lane maps: a stepped run proves the tiling and the addressing, only the device run
// proves the maps.  Every tensor a launch reads or writes is a copy allocated to its exact size (a read or write past it is a finding of the AddressSanitizer
// program tests/test_sr_cpu.py builds from this file and tests/sr_asan_main.cc); the workgroup's LDS image starts as pseudo-random bytes (lds_seed), as it does
// on the device.  hevc_amd/ never loads this library.
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "ingest_planes.h"
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
    bool take(const void *src, size_t bytes)
    {
        n = bytes;
        if (posix_memalign(&p, 16, bytes ? bytes : 16)) return false;
        if (src) memcpy(p, src, bytes);
        else memset(p, 0xA5, bytes);
        return true;
    }
};

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
    for (int wg = 0; wg <= nwg; wg++) {          // one past the last: must do nothing
        scramble(*sh);
        sr_conv_program<CIN, NB, PLANAR>(ex, *sh, a, wg);
    }
}
// the instances the product has (device.hip launch_sr_conv)
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
template <typename TI, bool FLT> void run_input(const SrInputArgs &a, int order)
{
    SeqExec ex;
    ex.order = order;
    const int f = a.unshuffle ? 2 : 1, nwg = sr_input_workgroups(a.sw / f, a.sh / f);
    for (int wg = 0; wg <= nwg; wg++) sr_input_program<TI, FLT>(ex, a, wg);
}
// the source planes placed as IngestSrcPlane does (exact end, alignment class `align`) and k_sr_input over them into `out`
template <typename TI, bool FLT> int input(const mihevc_rgb_format &f, int scale, int sw, int sh, const void *const *src, int align, uint16_t *out, int order)
{
    IngestSrcPlane<TI> sp[3];
    SrInputArgs a;
    const int planes = f.layout ? 1 : 3;
    for (int c = 0; c < 3; c++) {
        a.src[c] = nullptr;
        if (c >= planes) continue;
        if (!sp[c].place(src[c], f.layout ? f.layout * sw : sw, sh, align)) return -5;
        a.src[c] = sp[c].p;
    }
    a.out = out; a.pitch = sp[0].pitch; a.epp = f.layout ? f.layout : 1;
    a.pos[0] = f.r; a.pos[1] = f.g; a.pos[2] = f.b;
    a.vmax = f.sample ? 65535 : (1 << f.bit_depth) - 1;
    a.sw = sw; a.sh = sh; a.unshuffle = scale == 2;
    g_ingest_misaligned = 0;
    run_input<TI, FLT>(a, order);
    return g_ingest_misaligned ? -6 : 0;
}
int input_any(const mihevc_rgb_format &f, int scale, int sw, int sh, const void *const *src, int align, uint16_t *out, int order)
{
    if (f.sample == 2) return input<uint32_t, true>(f, scale, sw, sh, src, align, out, order);
    if (f.sample == 1) return input<uint16_t, true>(f, scale, sw, sh, src, align, out, order);
    if (f.bit_depth > 8) return input<uint16_t, false>(f, scale, sw, sh, src, align, out, order);
    return input<uint8_t, false>(f, scale, sw, sh, src, align, out, order);
}

}  // namespace

extern "C" {

// the workgroup's tile in output pixels, the input channels of a step and the output channels of a fragment
void emu_sr_tile(int *tw, int *th, int *k, int *m) { *tw = SR_TW; *th = SR_TH; *k = SR_K; *m = SR_M; }

// the flat weight count of a network, the device bytes of a source size, and the number of launches
int emu_sr_net_info(int scale, int blocks, int sw, int sh, unsigned long long *count, unsigned long long *bytes, int *launches)
{
    if ((scale != 2 && scale != 4) || blocks < 1) return -3;
    *count = sr_net_count(scale, blocks);
    *bytes = sr_geometry_ok(scale, sw, sh) ? sr_net_bytes(scale, sw, sh) : 0;
    *launches = 2 + blocks * 15 + 5;
    return 0;
}
// sr_pack_layer: weights [cout][cin][3][3] -> dst, 9 * cin_pad * cout_pad halves
void emu_sr_pack(const float *w, int cout, int cin, int cout_pad, int cin_pad, uint16_t *dst) { sr_pack_layer(w, cout, cin, cout_pad, cin_pad, dst); }
// float32 -> half of the packer and of the stepped epilogue
unsigned emu_sr_half(float f) { return sr_half_of_float_sw(f); }

// one launch: the arguments of mihevc_k_sr_conv, then the SeqExec thread order and the seed of the LDS images.  Returns 0, or -3
int emu_sr_conv(const mihevc_sr_conv_desc *d, const uint16_t *in, const float *weights, const float *bias, const uint16_t *r1, const uint16_t *r2, uint16_t *out,
                int order, unsigned lds_seed)
{
    if (!d || !in || !weights || !bias || !out || d->cin % SR_K || d->cin < SR_K || d->cin > SR_MAX_CIN) return -3;
    const int cout_pad = d->planar ? SR_M : d->cout, sw = d->up ? (d->width + 1) / 2 : d->width, sh = d->up ? (d->height + 1) / 2 : d->height;
    const size_t px = (size_t)d->width * d->height, out_n = px * (d->planar ? 3 : d->out_ch);
    std::vector<uint16_t> wpk(sr_packed_halves(cout_pad, d->cin));
    std::vector<float> b((size_t)cout_pad, 0.0f);
    sr_pack_layer(weights, d->cout, d->cin_real, cout_pad, d->cin, wpk.data());
    for (int c = 0; c < d->cout; c++) b[(size_t)c] = bias[c];
    Exact ein, ew, eb, e1, e2, eout;
    if (!ein.take(in, (size_t)sw * sh * d->in_ch * 2) || !ew.take(wpk.data(), wpk.size() * 2) || !eb.take(b.data(), b.size() * 4) || !eout.take(out, out_n * 2)) return -5;
    if (!e1.take(d->n_res >= 1 ? r1 : nullptr, d->n_res >= 1 ? px * d->r1_ch * 2 : 0) || !e2.take(d->n_res >= 2 ? r2 : nullptr, d->n_res >= 2 ? px * d->r2_ch * 2 : 0)) return -5;
    SrConvArgs a;
    a.in = (const uint16_t *)ein.p; a.out = (uint16_t *)eout.p; a.wpk = (const uint16_t *)ew.p; a.bias = (const float *)eb.p;
    a.r1 = (const uint16_t *)e1.p; a.r2 = (const uint16_t *)e2.p;
    a.in_ch = d->in_ch; a.in_off = d->in_off; a.out_ch = d->out_ch; a.out_off = d->out_off; a.r1_ch = d->r1_ch; a.r1_off = d->r1_off; a.r2_ch = d->r2_ch; a.r2_off = d->r2_off;
    a.w = d->width; a.h = d->height; a.up = d->up; a.act = d->act; a.n_res = d->n_res; a.slope = d->slope; a.a1 = d->a1; a.a2 = d->a2;
    g_lds_rnd = 0x9E3779B97F4A7C15ull ^ lds_seed;
    if (int e = conv(a, d->cin, cout_pad, d->planar != 0, order)) return e;
    memcpy(out, eout.p, out_n * 2);
    return 0;
}

// k_sr_input: the arguments of mihevc_k_sr_input with tight rows (pitch = row), then the alignment class of the placed planes and the thread order
int emu_sr_input(const mihevc_rgb_format *fmt, int scale, int sw, int sh, const void *p0, const void *p1, const void *p2, int align, uint16_t *out, int order)
{
    if (!rgb_format_ok(fmt) || (scale != 2 && scale != 4) || !sr_geometry_ok(scale, sw, sh) || !out) return -3;
    const int f = scale == 2 ? 2 : 1;
    Exact eo;
    const size_t n = (size_t)(sw / f) * (sh / f) * SR_CIN0 * 2;
    if (!eo.take(nullptr, n)) return -5;
    const void *src[3] = {p0, p1, p2};
    if (int e = input_any(*fmt, scale, sw, sh, src, align, (uint16_t *)eo.p, order)) return e;
    memcpy(out, eo.p, n);
    return 0;
}

// the whole network as mihevc_k_sr_network runs it: k_sr_input, then every launch of the list over an arena of exactly sr_net_bytes
int emu_sr_network(const mihevc_sr_model *model, const float *weights, size_t count, const mihevc_rgb_format *fmt, int sw, int sh, const void *p0, const void *p1,
                   const void *p2, uint16_t *out, int order, unsigned lds_seed)
{
    if (!sr_model_ok(model) || !rgb_format_ok(fmt) || !sr_geometry_ok(model->scale, sw, sh) || !out) return -3;
    SrNet net;
    if (!sr_net_build(model->scale, model->blocks, weights, count, net)) return -3;
    const int f = model->scale == 2 ? 2 : 1, tw = sw / f, th = sh / f;
    size_t off[SR_BUFS];
    Exact arena;
    if (!arena.take(nullptr, sr_arena_layout(tw, th, off)) || arena.n != sr_net_bytes(model->scale, sw, sh)) return -5;
    const void *src[3] = {p0, p1, p2};
    if (int e = input_any(*fmt, model->scale, sw, sh, src, 16, (uint16_t *)((uint8_t *)arena.p + off[SR_X]), order)) return e;
    g_lds_rnd = 0x9E3779B97F4A7C15ull ^ lds_seed;
    if (int e = sr_for_each_launch(net, (uint8_t *)arena.p, net.wpk.data(), net.bias.data(), tw, th,
                                   [&](int cin, int cout, bool planar, const SrConvArgs &a) { return conv(a, cin, cout, planar, order); })) return e;
    memcpy(out, (uint8_t *)arena.p + off[SR_OUT], (size_t)tw * th * 16 * 3 * 2);
    return 0;
}

}  // extern "C"
