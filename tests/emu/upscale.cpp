// tests/emu/upscale.cpp — TEST HARNESS, NOT PRODUCT (part of tests/emu/libkernel_emu.so).  The upscaling program of hevc_amd/csrc/kernels/upscale.h (k_upscale)
// stepped on the CPU with the sequential executor, every workgroup of the launch, over the tables of hevc_amd/csrc/scale_taps.h (scale_taps_build_up), which it
// also hands out as they are.  Source planes and output planes are those of the stepped converters (ingest_planes.h): sources allocated to their exact size
// with the alignment the case asks for (a read past them is a finding of the AddressSanitizer program tests/test_upscale_cpu.py builds from this file and
// tests/upscale_asan_main.cc), outputs garbage-filled.  The workgroup's LDS images start as pseudo-random bytes (lds_seed), as they do on the device.
// hevc_amd/ never loads this library.
#include <memory>
#include <vector>

#include "ingest_planes.h"
#include "../../hevc_amd/csrc/kernels/upscale.h"
#include "../../hevc_amd/csrc/scale_taps.h"

using namespace mihevc;

namespace {

template <typename TI, typename TO>
int run(const mihevc_upscale_src &f, const void *const *src, int dw, int dh, int out_depth, int order, int align, unsigned lds_seed, void *const *out, int *stats)
{
    const int pw = (dw + 7) & ~7, ph = (dh + 7) & ~7;
    UpscaleBlock blk;
    if (!upscale_block_build(f.width, f.height, dw, dh, UP_TH, UP_HALO, UP_ROWS, blk)) return -3;
    IngestSrcPlane<TI> sp[3];
    for (int c = 0; c < 3; c++)
        if (!sp[c].place(src[c], c ? f.width / 2 : f.width, c ? f.height / 2 : f.height, align)) return -5;
    IngestOutPlanes<TO> op(pw, ph);
    const int32_t *first[4], *near[4];
    const int16_t *coef[4];
    for (int k = 0; k < 4; k++) {
        first[k] = (const int32_t *)(blk.bytes.data() + blk.first[k]); near[k] = (const int32_t *)(blk.bytes.data() + blk.near[k]);
        coef[k] = (const int16_t *)(blk.bytes.data() + blk.coef[k]);
    }
    const UpscaleArgs a = upscale_args(f, sp[0].p, sp[1].p, sp[2].p, sp[0].pitch, sp[1].pitch, dw, dh, pw, ph, out_depth, op.dst, op.stride, first, near, coef);
    stats[2] = ingest_align(a.src[0], (size_t)a.pitch[0] * sizeof(TI)); stats[3] = ingest_align(a.src[1], (size_t)a.pitch[1] * sizeof(TI));
    SeqExec ex;
    ex.order = order;
    g_ingest_misaligned = 0;
    std::unique_ptr<UpscaleShared> sh(new UpscaleShared);
    unsigned long long x = 0x9E3779B97F4A7C15ull ^ lds_seed;
    const int nwg = upscale_workgroups(pw, ph);
    for (int wg = 0; wg < nwg; wg++) {
        unsigned char *b = (unsigned char *)sh.get();
        for (size_t i = 0; i < sizeof(UpscaleShared); i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; b[i] = (unsigned char)(x >> 32); }
        upscale_tile_program<TI, TO>(ex, *sh, a, wg);
    }
    int wg_past = nwg;
    stats[0] = g_ingest_misaligned + (upscale_locate(pw, ph, wg_past) != -1);
    stats[1] = op.copy_back(out);
    return 0;
}

}  // namespace

extern "C" {

// the workgroup's tile in output samples, its halo and the rows of its LDS image: a test picks sizes the tile does not divide
void emu_upscale_tile(int *tw, int *th, int *halo, int *rows) { *tw = UP_TW; *th = UP_TH; *halo = UP_HALO; *rows = UP_ROWS; }

// scale_taps_build_up(S, Dn, p): first[Dn], near[Dn], coef[Dn * 4], *taps.  Returns 0, or -3 when the builder refuses
int emu_upscale_taps(int S, int Dn, int p, int32_t *first, int32_t *near, int16_t *coef, int *taps)
{
    UpscaleTaps t;
    if (!scale_taps_build_up(S, Dn, p, t)) return -3;
    memcpy(first, t.first.data(), t.first.size() * sizeof(int32_t));
    memcpy(near, t.near.data(), t.near.size() * sizeof(int32_t));
    memcpy(coef, t.coef.data(), t.coef.size() * sizeof(int16_t));
    *taps = t.taps;
    return 0;
}

// whether the four tables of a size pair fit the kernel (upscale_block_build): 0, or -3
int emu_upscale_block(int sw, int sh, int dw, int dh)
{
    UpscaleBlock blk;
    return upscale_block_build(sw, sh, dw, dh, UP_TH, UP_HALO, UP_ROWS, blk) ? 0 : -3;
}

// src: the source's size, depth and settings; y, u, v: its tight planes (pitch = row); dw x dh: display size of the output; out_*: tight planes of the coded
// size, uint8 at out_depth 8, uint16 at 10; order: SeqExec thread order; align: 16 / 8 / 4 / 1 (IngestSrcPlane); lds_seed: of the LDS images' initial bytes.
// stats[0]: misaligned accesses (must be 0), stats[1]: samples written outside the coded width (must be 0), stats[2], stats[3]: the alignment class of the
// luma / chroma planes the kernel read.  Returns 0, or -3
int emu_upscale(const mihevc_upscale_src *src, const void *y, const void *u, const void *v, int dw, int dh, int out_depth, int order, int align, unsigned lds_seed,
                void *out_y, void *out_u, void *out_v, int *stats)
{
    if (!upscale_src_ok(src) || !upscale_geometry_ok(src->width, src->height, dw, dh) || (out_depth != 8 && out_depth != 10)) return -3;
    if (align != 16 && align != 8 && align != 4 && align != 1) return -3;
    const void *p[3] = {y, u, v};
    void *out[3] = {out_y, out_u, out_v};
    const bool in16 = src->bit_depth > 8, out16 = out_depth > 8;
    if (in16 && out16) return run<uint16_t, uint16_t>(*src, p, dw, dh, out_depth, order, align, lds_seed, out, stats);
    if (in16) return run<uint16_t, uint8_t>(*src, p, dw, dh, out_depth, order, align, lds_seed, out, stats);
    if (out16) return run<uint8_t, uint16_t>(*src, p, dw, dh, out_depth, order, align, lds_seed, out, stats);
    return run<uint8_t, uint8_t>(*src, p, dw, dh, out_depth, order, align, lds_seed, out, stats);
}

}  // extern "C"
