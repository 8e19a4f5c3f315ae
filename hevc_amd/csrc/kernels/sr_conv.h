// hevc_amd/csrc/kernels/sr_conv.h — learned super-resolution (mihevc_send_frame_sr, mihevc_k_sr_conv, mihevc_k_sr_network): the two kernels an RRDBNet needs.
// The numerical definition is DESIGN.md §6l (normative); csrc/sr_net.h packs the weights and lists the launches of a network.
//   tensors     activations are IEEE halves, NHWC: pixel (y, x) of a tensor of C channels starts at element (y w + x) C.  A launch reads `cin` channels from
//               channel `in_off` on and writes `cout` from `out_off` on, so the concatenations of a dense block are slices of one buffer of 192 channels.
//               Offsets and channel counts of a buffer are multiples of 8 (16-byte loads) and the base is 16-byte aligned
//   k_sr_conv   out[y][x][co] = E(bias[co] + sum over ky, kx, ci of in[y + ky - 1][x + kx - 1][ci] W[co][ci][ky][kx]), zero outside the picture.  With `up`
//               the input is the source enlarged by nearest 2x and never stored: position (yy, xx) of the enlarged picture reads the source at
//               (yy >> 1, xx >> 1).  Products of halves are summed in fp32 by the MFMA, in the hardware's order
//   epilogue    E, in fp32: v = acc + bias; act: v = v >= 0 ? v : slope v; n_res >= 1: v = v a1 + r1; n_res == 2: v = v a2 + r2 (r: halves of the output's
//               pixel, widened); v is rounded to half (nearest even) once.  The compiler may contract v a + r into one fma: the definition allows either
//   planar      the last layer: channels 0 .. 2 go to three planes of w x h halves, one after the other, instead of NHWC
//   k_sr_input  a source as mihevc_send_frame_rgb takes it -> the network's input tensor of SR_CIN0 channels in [0, 1]: integers v = min(r, 2^B - 1),
//               x = half(float32(v) / float32(2^B - 1)) (a correctly rounded float32 division, then nearest even); floats x = half(min(max(x, 0), 1)), NaN 0.
//               Scale 4: channels R, G, B.  Scale 2: the pixel-unshuffle, channel c 4 + dy 2 + dx at (y, x) is component c at (2 y + dy, 2 x + dx).  The other
//               channels are written as zeros: they meet zero weights, and a NaN there would still poison the sum
// k_sr_conv is an implicit GEMM on v_mfma_f32_16x16x32_f16.  The 16x16x32 shape, not 32x32x16: its K of 32 is the growth of a dense block, so every Cin of the
// network is a whole number of steps; four accumulators per 16 x 16 result let a wave hold a 64-channel x 32-pixel tile in 32 registers; and a lane's fragment
// is the same 16 bytes either way.  The WEIGHTS are the A operand (rows = output channels) and the pixels the B operand (columns = 16 adjacent pixels of a
// row), so that a lane's four results are four adjacent channels of one pixel: one 8-byte store, and 8-byte loads of the residuals.
// A workgroup computes SR_TW x SR_TH output pixels times every output channel of the launch:
//   phase 1   the input tile with its one-pixel halo, all `cin` channels, into LDS: 16-byte global loads, zeros outside the picture (the padding), rows of
//             CIN halves + 16 bytes.  That pitch does NOT keep the 16 pixels of a fragment read off each other's banks: measured, bank-conflict cycles are 2.2 x the
//             cycles LDS instructions are active at 64 -> 32 and one per MFMA at 192 -> 64; a swizzled image would
//   phase 2   (mfma_phase) wave q takes rows 2q and 2q + 1 of the tile.  Step s = tap * CIN / 32 + chunk: the pixel fragments are one ds_read_b128 each, the
//             weight fragments one 16-byte global load each from the packed block (sr_net.h: [step][tile of 16 channels][lane]), 2 NB MFMAs.  Then the epilogue
// What this costs: with Cout = 32 a step is 2 LDS reads and 2 global loads for 4 MFMAs of 16 cycles, and every wave of a workgroup fetches the same weights
// (from L1 / L2): the kernel is bound by its loads, not by the matrix unit (DESIGN.md §6l has the measurements and what would have to change).
// The stepped run (tests/emu/sr.cpp, SeqExec::mfma_phase) proves the tiling and the addressing; only the device run proves the lane maps.
// The compact networks (SRVGGNetCompact, realesr-general) have a kernel of their own, sr_compact.h.  Out of scope: other architectures, scale 1,
// num_feat / num_grow_ch other than 64 / 32, tiling a frame, batching frames, fp8 / int8 weights.
#pragma once
#include "ingest_rgb.h"

namespace mihevc {

constexpr int SR_TW = 16, SR_TH = 8;                      // the tile: 16 pixels are the columns of one MFMA, a wave takes two rows
constexpr int SR_HW = SR_TW + 2, SR_HH = SR_TH + 2;       // with the halo
constexpr int SR_K = 32, SR_M = 16;                       // input channels per step, output channels per weight fragment
constexpr int SR_ROWS = SR_TH / (NT / 64);                // rows per wave
constexpr int SR_CIN0 = 32;                               // channels of the input tensor (3 or 12 real)
constexpr int SR_MAX_CIN = 192;
constexpr int SR_PER_CU = 2;                              // the second launch bound: 2 x 69 KB of LDS at CIN = 192

template <int CIN> struct SrShared {
    uint8_t in[SR_HH * SR_HW][CIN * 2 + 16];              // 72,000 bytes at CIN = 192; 14,400 at 32
};

struct SrConvArgs {
    const uint16_t *in;             // source tensor (with `up`: of ((h + 1) >> 1) x ((w + 1) >> 1) pixels)
    uint16_t *out;                  // NHWC, or the first of three planes
    const uint16_t *wpk;            // packed weights of the layer (sr_pack_layer)
    const float *bias;              // NB * 16 of them
    const uint16_t *r1, *r2;
    int in_ch, in_off, out_ch, out_off, r1_ch, r1_off, r2_ch, r2_off;      // channels of the buffer, first channel of the slice
    int w, h;                       // output size
    int up, act, n_res;
    float slope, a1, a2;
};

struct SrInputArgs {
    const void *src[3];             // three planes, or the packed plane in src[0]
    uint16_t *out;                  // SR_CIN0 channels
    int pitch, epp;                 // elements per row; elements per pixel in a row: 1 (planes), 3, 4
    int pos[3];                     // R, G, B: plane index, or element index inside the pixel
    int vmax;
    int sw, sh;                     // source size
    int unshuffle;                  // 1: scale 2
};

HDI int sr_conv_workgroups(int w, int h) { return ((w + SR_TW - 1) / SR_TW) * ((h + SR_TH - 1) / SR_TH); }
HDI int sr_input_workgroups(int tw, int th) { return (tw * th + NT - 1) / NT; }

// float32 -> half, nearest even, in integers: what v_cvt_f16_f32 does (overflow to infinity, subnormal halves kept)
HDI uint16_t sr_half_of_float_sw(float f)
{
    uint32_t x;
    __builtin_memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (x > 0x7f800000u ? 0x200u : 0u));
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);
    if (x < 0x38800000u) {
        if (x <= 0x33000000u) return (uint16_t)sign;
        const uint32_t m = (x & 0x7fffffu) | 0x800000u, shift = 126u - (x >> 23), rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
        uint32_t r = m >> shift;
        if (rem > half || (rem == half && (r & 1u))) r++;
        return (uint16_t)(sign | r);
    }
    uint32_t r = (x - 0x38000000u) >> 13;
    const uint32_t rem = x & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) r++;
    return (uint16_t)(sign | r);
}
DEV uint32_t sr_half_of_float(float f)
{
#if MIHEVC_GPU && defined(__HIP_DEVICE_COMPILE__)
    const _Float16 h = (_Float16)f;
    uint16_t b;
    __builtin_memcpy(&b, &h, 2);
    return b;
#else
    return sr_half_of_float_sw(f);
#endif
}

// workgroup `wg` of a launch.  NB: fragments of 16 output channels (Cout = 16 NB; PLANAR: one, of which three channels are stored)
template <int CIN, int NB, bool PLANAR, class Ex> DEV void sr_conv_program(Ex &ex, SrShared<CIN> &s, const SrConvArgs &a, int wg)
{
    static_assert(CIN % SR_K == 0 && CIN <= SR_MAX_CIN && NB >= 1 && (!PLANAR || NB == 1), "shape");
    constexpr int KC = CIN / SR_K, CHUNKS = CIN / 8;
    const int w = a.w, h = a.h, up = a.up;
    const int ntx = (w + SR_TW - 1) / SR_TW, ty = wg / ntx, tx = wg - ty * ntx;
    if (ty * SR_TH >= h) return;
    const int x_base = tx * SR_TW, y_base = ty * SR_TH;
    const int sw = up ? (w + 1) >> 1 : w;
    const uint16_t *const in = a.in + a.in_off;
    const int in_ch = a.in_ch;
    ex.phase([&](int tid) {          // the tile and its halo: chunk c (8 channels) of halo pixel p
        for (int i = tid; i < SR_HH * SR_HW * CHUNKS; i += NT) {
            const int p = i / CHUNKS, c = i - p * CHUNKS, py = p / SR_HW, y = y_base - 1 + py, x = x_base - 1 + (p - py * SR_HW);
            mfma_frag v = {0u, 0u, 0u, 0u};
            if (y >= 0 && y < h && x >= 0 && x < w) {
                const ptrdiff_t pix = (ptrdiff_t)(y >> up) * sw + (x >> up);
                v = *(const mfma_frag *)__builtin_assume_aligned(in + pix * in_ch + c * 8, 16);
            }
            *(mfma_frag *)__builtin_assume_aligned(&s.in[p][c * 16], 16) = v;
        }
    });
    const uint16_t *const wpk = a.wpk;
    const float *const bias = a.bias;
    uint16_t *const out = a.out;
    const uint16_t *const r1 = a.r1, *const r2 = a.r2;
    const int out_ch = a.out_ch, out_off = a.out_off, r1_ch = a.r1_ch, r1_off = a.r1_off, r2_ch = a.r2_ch, r2_off = a.r2_off, act = a.act, n_res = a.n_res;
    const float slope = a.slope, a1 = a.a1, a2 = a.a2;
    ex.template mfma_phase<NB, SR_ROWS>(9 * KC,
        [&](int tid, int step, mfma_frag (&fw)[NB], mfma_frag (&fp)[SR_ROWS]) {
            const int lane = tid & 63, row0 = (tid >> 6) * SR_ROWS, tap = step / KC, kc = step - tap * KC, ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
            for (int m = 0; m < SR_ROWS; m++)
                fp[m] = *(const mfma_frag *)__builtin_assume_aligned(&s.in[(row0 + m + ky) * SR_HW + (lane & 15) + kx][(kc * SR_K + 8 * (lane >> 4)) * 2], 16);
#pragma unroll
            for (int n = 0; n < NB; n++)
                fw[n] = *(const mfma_frag *)__builtin_assume_aligned(wpk + ((ptrdiff_t)(step * NB + n) * 64 + lane) * 8, 16);
        },
        [&](int tid, const mfma_acc (&acc)[NB][SR_ROWS]) {
            const int lane = tid & 63, x = x_base + (lane & 15), c0 = 4 * (lane >> 4);
            if (x >= w) return;
#pragma unroll
            for (int m = 0; m < SR_ROWS; m++) {
                const int y = y_base + (tid >> 6) * SR_ROWS + m;
                if (y >= h) continue;
                const ptrdiff_t pix = (ptrdiff_t)y * w + x;
#pragma unroll
                for (int n = 0; n < NB; n++) {
                    const int co = n * SR_M + c0;
                    float v[4];
                    ingest_u32x2 q1 = {0u, 0u}, q2 = {0u, 0u};
                    if (n_res >= 1) q1 = *(const ingest_u32x2 *)__builtin_assume_aligned(r1 + pix * r1_ch + r1_off + co, 8);
                    if (n_res >= 2) q2 = *(const ingest_u32x2 *)__builtin_assume_aligned(r2 + pix * r2_ch + r2_off + co, 8);
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        v[i] = acc[n][m][i] + bias[co + i];
                        if (act) v[i] = v[i] >= 0.0f ? v[i] : slope * v[i];
                        if (n_res >= 1) v[i] = v[i] * a1 + half_bits_to_float((q1[i >> 1] >> (16 * (i & 1))) & 0xffffu);
                        if (n_res >= 2) v[i] = v[i] * a2 + half_bits_to_float((q2[i >> 1] >> (16 * (i & 1))) & 0xffffu);
                    }
                    if constexpr (PLANAR) {
                        if (c0 == 0)
#pragma unroll
                            for (int i = 0; i < 3; i++) out[(ptrdiff_t)i * w * h + pix] = (uint16_t)sr_half_of_float(v[i]);
                    } else {
                        const ingest_u32x2 o = {sr_half_of_float(v[0]) | sr_half_of_float(v[1]) << 16, sr_half_of_float(v[2]) | sr_half_of_float(v[3]) << 16};
                        *(ingest_u32x2 *)__builtin_assume_aligned(out + pix * out_ch + out_off + co, 8) = o;
                    }
                }
            }
        });
}

// the value of a raw element as the half the network reads
template <typename TI, bool FLT> DEV uint32_t sr_input_half(int raw, int vmax)
{
    if constexpr (!FLT) return sr_half_of_float((float)imin(raw, vmax) / (float)vmax);
    else {
        float x = sizeof(TI) == 2 ? rgb_float_of_half((uint32_t)raw) : rgb_float_of_bits((uint32_t)raw);
        x = x > 0.0f ? x : 0.0f;      // NaN compares false: 0
        x = x < 1.0f ? x : 1.0f;
        return sr_half_of_float(x);
    }
}
// workgroup `wg`: NT pixels of the input tensor, one a lane
template <typename TI, bool FLT, class Ex> DEV void sr_input_program(Ex &ex, const SrInputArgs &a, int wg)
{
    const int f = a.unshuffle ? 2 : 1, tw = a.sw / f, th = a.sh / f;
    ex.phase([&](int tid) {
        const int p = wg * NT + tid;
        if (p >= tw * th) return;
        const int y = p / tw, x = p - y * tw;
        uint32_t hv[12];
#pragma unroll
        for (int k = 0; k < 12; k++) hv[k] = 0;
        for (int c = 0; c < 3; c++)
            for (int d = 0; d < f * f; d++) {
                const int sy = y * f + (d >> 1), sx = x * f + (d & 1);      // (f == 1: d == 0)
                const TI *e = a.epp == 1 ? (const TI *)a.src[a.pos[c]] + (ptrdiff_t)sy * a.pitch + sx : (const TI *)a.src[0] + (ptrdiff_t)sy * a.pitch + (ptrdiff_t)sx * a.epp + a.pos[c];
                int raw;
                ingest_element(e, raw);
                const uint32_t hb = sr_input_half<TI, FLT>(raw, a.vmax);
                const int ch = f == 2 ? c * 4 + d : c;
#pragma unroll
                for (int k = 0; k < 12; k++)      // (no indexing of registers by ch)
                    if (k == ch) hv[k] = hb;
            }
        uint16_t *o = a.out + (ptrdiff_t)p * SR_CIN0;
#pragma unroll
        for (int q = 0; q < SR_CIN0 / 8; q++) {
            mfma_frag v = {0u, 0u, 0u, 0u};
            if (q == 0) v = mfma_frag{hv[0] | hv[1] << 16, hv[2] | hv[3] << 16, hv[4] | hv[5] << 16, hv[6] | hv[7] << 16};
            if (q == 1) v = mfma_frag{hv[8] | hv[9] << 16, hv[10] | hv[11] << 16, 0u, 0u};
            *(mfma_frag *)__builtin_assume_aligned(o + q * 8, 16) = v;
        }
    });
}

}  // namespace mihevc
