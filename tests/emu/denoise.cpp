// tests/emu/denoise.cpp — TEST HARNESS, NOT PRODUCT (part of tests/emu/libkernel_emu.so).  The denoising program of hevc_amd/csrc/kernels/denoise.h (k_denoise) stepped
// on the CPU with the sequential executor, every workgroup of the launch.  Source planes and output planes are those of the stepped converters
// (ingest_planes.h): the nine source planes allocated to their exact size with the alignment the case asks for (a read past them is a finding of the
// AddressSanitizer program tests/test_denoise_cpu.py builds from this file and tests/denoise_asan_main.cc), outputs garbage-filled.  The workgroup's LDS images
// start as pseudo-random bytes (lds_seed), as they do on the device.  hevc_amd/ never loads this library.
#include <memory>

#include "ingest_planes.h"
#include "../../hevc_amd/csrc/kernels/denoise.h"

using namespace mihevc;

namespace {

template <typename T>
int run(const mihevc_denoise &dn, const void *const *prev, const void *const *cur, const void *const *next, int w, int h, int depth, int order, int align, unsigned lds_seed,
        void *const *out, int *stats)
{
    const int pw = (w + 7) & ~7, ph = (h + 7) & ~7;
    IngestSrcPlane<T> sp[3][3];
    const void *p[3][3];
    for (int f = 0; f < 3; f++)
        for (int c = 0; c < 3; c++) {
            if (!sp[f][c].place((f == 0 ? prev : f == 1 ? cur : next)[c], c ? w / 2 : w, c ? h / 2 : h, align)) return -5;
            p[f][c] = sp[f][c].p;
        }
    IngestOutPlanes<T> op(pw, ph);
    const DenoiseArgs a = denoise_args(dn, depth, p[0], p[1], p[2], sp[0][0].pitch, sp[0][1].pitch, w, h, pw, ph, op.dst, op.stride);
    stats[2] = a.f.align[0]; stats[3] = a.f.align[1];
    SeqExec ex;
    ex.order = order;
    g_ingest_misaligned = 0;
    std::unique_ptr<DenoiseShared> sh(new DenoiseShared);
    unsigned long long x = 0x9E3779B97F4A7C15ull ^ lds_seed;
    const int nwg = deint_workgroups(pw, ph);
    for (int wg = 0; wg < nwg; wg++) {
        unsigned char *b = (unsigned char *)sh.get();
        for (size_t i = 0; i < sizeof(DenoiseShared); i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; b[i] = (unsigned char)(x >> 32); }
        denoise_tile_program<T>(ex, *sh, a, wg);
    }
    int wg_past = nwg;
    stats[0] = g_ingest_misaligned + (deint_locate(pw, ph, wg_past) != -1);
    stats[1] = op.copy_back(out);
    return 0;
}

}  // namespace

extern "C" {

// the workgroup's tile in output samples and the bytes of its LDS images
void emu_denoise_tile(int *tw, int *th, int *lds_bytes) { *tw = DN_TW; *th = DN_TH; *lds_bytes = (int)sizeof(DenoiseShared); }

// the kernel's own division (denoise_div) against the language's over the whole range of the definition: every divisor 1 .. 11 * 1020, and for every quotient up to
// the 10-bit peak the numerators at its lower end, in its middle and at its upper end, below 2^24.  Returns the number of wrong quotients
int emu_denoise_div_check()
{
    int bad = 0;
    for (int w = 1; w <= 11 * 1020; w++)
        for (int q = 0; q <= 1023; q++)
            for (int n : {q * w, q * w + w / 2, q * w + w - 1})
                if (n < (1 << 24)) bad += denoise_div(n, w) != n / w;
    return bad;
}

// dn: the four strengths; prev / cur / next: Y, Cb, Cr of three frames of w x h samples as tight planes (pitch = row), uint8 at depth 8, uint16 at 10; out_*: tight
// planes of the coded size; order: SeqExec thread order; align: 16 / 8 / 4 / 1 (IngestSrcPlane); lds_seed: of the LDS images' initial bytes.  stats[0]:
// misaligned accesses (must be 0), stats[1]: samples written outside the coded width (must be 0), stats[2], stats[3]: the alignment class of the luma / chroma
// planes the kernel read.  Returns 0, or -3 for what mihevc_k_denoise refuses
int emu_denoise(const mihevc_denoise *dn, const void *const *prev, const void *const *cur, const void *const *next, int w, int h, int depth, int order, int align,
                unsigned lds_seed, void *out_y, void *out_u, void *out_v, int *stats)
{
    if (!denoise_strength_ok(dn) || !denoise_geometry_ok(w, h) || (depth != 8 && depth != 10)) return -3;
    if (align != 16 && align != 8 && align != 4 && align != 1) return -3;
    void *out[3] = {out_y, out_u, out_v};
    if (depth > 8) return run<uint16_t>(*dn, prev, cur, next, w, h, depth, order, align, lds_seed, out, stats);
    return run<uint8_t>(*dn, prev, cur, next, w, h, depth, order, align, lds_seed, out, stats);
}

}  // extern "C"
