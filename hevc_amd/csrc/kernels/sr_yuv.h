// hevc_amd/csrc/kernels/sr_yuv.h — a Y'CbCr source in front of the learned super-resolution (mihevc_send_frame_sr_yuv, mihevc_k_sr_from_yuv): a planar 4:2:0
// Y'CbCr picture -> the network's input tensor, the 32 half channels NHWC that k_sr_input (sr_conv.h) writes for an R'G'B' source.  The definition (normative;
// DESIGN.md §6l repeats it); everything up to the division is in integers:
//   source    W x H, both even, each at least 4.  B = 8, 10 or 12; elements uint8 at B = 8, else little-endian uint16, lsb aligned, v = min(r, 2^B - 1).  Matrix
//             code 1, 5, 6 or 9, limited or full range
//   1 chroma to the luma grid: step 1 of the colour table (lut3d.h), unchanged: h(i, 2x) = 2 c[i][x], h(i, 2x+1) = c[i][x] + c[i][min(x+1, W/2-1)];
//             row 2j: C8 = 3 h(j, .) + h(max(j-1, 0), .); row 2j+1: C8 = 3 h(j, .) + h(min(j+1, H/2-1), .): a factor 8 carried, no rounding
//   2 Y'CbCr -> R'G'B' at 16 bit: step 2 of the colour table, unchanged: the five coefficients of lut3d_inverse, sums in 64 bits,
//             v = clip((t + 2^15) >> 16, 0, 65535) (lut_rgb16, the one copy of it)
//   3 to half x = half(float32(v) / float32(65535)): k_sr_input's rule for integers at B = 16, a correctly rounded fp32 division, then nearest even
//   channels  scale 4: a tensor of W x H pixels, channels 0 .. 2 are R, G, B, the other 29 are written as zeros.  Scale 2: a tensor of W/2 x H/2 pixels, the
//             pixel-unshuffle of §6l: channel c 4 + dy 2 + dx at (y, x) is component c at (2y + dy, 2x + dx); 12 real channels, 20 zeros
// One launch per picture (k_sr_from_yuv), no LDS.  A lane owns the luma block of columns 2i, 2i+1 and rows 2j, 2j+1: the pixels that share chroma row j with
// weight 3 (at scale 2 they are one pixel of the tensor, at scale 4 four).  It reads chroma columns i and min(i+1, W/2-1) of rows j-1, j, j+1 (clamped) once,
// forms the two h values of each row once and serves its four pixels from them; every element goes through ingest_element, behind ingest.h's one access hook,
// so a plane needs no more than the alignment of its element and any pitch will do.  The stores are the 16-byte fragments k_sr_input writes.  The traffic is
// the tensor's: 64 bytes stored per pixel at scale 4 against 1.5 to 3 read.
#pragma once
#include "lut3d.h"
#include "sr_conv.h"

namespace mihevc {

struct SrYuvArgs {
    const void *src[3];      // Y, Cb, Cr
    uint16_t *out;           // SR_CIN0 channels, 16-byte aligned
    int pitch[3];            // in elements
    int sw, sh;              // source size
    int unshuffle;           // 1: scale 2
    int vmax, oY, oC8;       // as Lut3dArgs: v = min(r, vmax); y = Y - oY; cb = Cb8 - oC8
    int nY, nRv, nGu, nGv, nBu;
};

HDI bool sr_yuv_src_ok(const mihevc_sr_yuv *f)
{
    if (!f || (f->bit_depth != 8 && f->bit_depth != 10 && f->bit_depth != 12) || !rgb_matrix_ok(f->matrix) || (f->full_range != 0 && f->full_range != 1)) return false;
    if (f->reserved[0] | f->reserved[1] | f->reserved[2]) return false;
    return f->width >= 4 && f->height >= 4 && f->width <= 8192 && f->height <= 8192 && !((f->width | f->height) & 1);
}
// the planes are there and aligned to their element, and the pitches (elements) hold a row
HDI bool sr_yuv_planes_ok(const mihevc_sr_yuv &f, const void *y, const void *u, const void *v, int pitch_y, int pitch_c)
{
    const unsigned es = f.bit_depth > 8 ? 2 : 1;
    if (!y || !u || !v || (uintptr_t)y % es || (uintptr_t)u % es || (uintptr_t)v % es) return false;
    return pitch_y >= f.width && pitch_c >= f.width / 2;
}
HDI int sr_yuv_workgroups(int sw, int sh) { return ((sw / 2) * (sh / 2) + NT - 1) / NT; }
// every field from the source's description and the planes; out: the tensor
inline SrYuvArgs sr_yuv_args(const mihevc_sr_yuv &f, int scale, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, uint16_t *out)
{
    SrYuvArgs a;
    a.src[0] = y; a.src[1] = u; a.src[2] = v; a.out = out;
    a.pitch[0] = pitch_y; a.pitch[1] = a.pitch[2] = pitch_c;
    a.sw = f.width; a.sh = f.height; a.unshuffle = scale == 2;
    a.vmax = (1 << f.bit_depth) - 1; a.oY = f.full_range ? 0 : 16 << (f.bit_depth - 8); a.oC8 = 8 << (f.bit_depth - 1);
    int c[5];
    lut3d_inverse(f.matrix, f.full_range != 0, f.bit_depth, c);
    a.nY = c[0]; a.nRv = c[1]; a.nGu = c[2]; a.nGv = c[3]; a.nBu = c[4];
    return a;
}

template <typename TI> DEV int sr_yuv_element(const SrYuvArgs &a, const TI *p)
{
    int v;
    ingest_element(p, v);
    return imin(v, a.vmax);
}
// workgroup `wg`: NT blocks of 2 x 2 luma samples, one a lane
template <typename TI, class Ex> DEV void sr_from_yuv_program(Ex &ex, const SrYuvArgs &a, int wg)
{
    const int bw = a.sw / 2, bh = a.sh / 2;
    ex.phase([&](int tid) {
        const int b = wg * NT + tid;
        if (b >= bw * bh) return;
        const int j = b / bw, i = b - j * bw, i1 = imin(i + 1, bw - 1), ju = imax(j - 1, 0), jd = imin(j + 1, bh - 1);
        // step 1: per component the h values of columns 2i and 2i + 1 in rows j (weight 3), j - 1 and j + 1, then C8[c][row of the block][column of the block]
        int C8[2][2][2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const TI *const pl = (const TI *)a.src[1 + c];
            const TI *const rn = pl + (ptrdiff_t)j * a.pitch[1 + c], *const ru = pl + (ptrdiff_t)ju * a.pitch[1 + c], *const rd = pl + (ptrdiff_t)jd * a.pitch[1 + c];
            const int n0 = sr_yuv_element(a, rn + i), n1 = sr_yuv_element(a, rn + i1);
            const int u0 = sr_yuv_element(a, ru + i), u1 = sr_yuv_element(a, ru + i1);
            const int d0 = sr_yuv_element(a, rd + i), d1 = sr_yuv_element(a, rd + i1);
            const int hn[2] = {2 * n0, n0 + n1}, hu[2] = {2 * u0, u0 + u1}, hd[2] = {2 * d0, d0 + d1};
#pragma unroll
            for (int k = 0; k < 2; k++) { C8[c][0][k] = 3 * hn[k] + hu[k]; C8[c][1][k] = 3 * hn[k] + hd[k]; }
        }
        // steps 2 and 3: hv[component][row][column]
        uint32_t hv[3][2][2];
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const TI *const ry = (const TI *)a.src[0] + (ptrdiff_t)(2 * j + r) * a.pitch[0] + 2 * i;
#pragma unroll
            for (int k = 0; k < 2; k++) {
                int v[3];
                lut_rgb16(a, sr_yuv_element(a, ry + k), C8[0][r][k], C8[1][r][k], v);
#pragma unroll
                for (int c = 0; c < 3; c++) hv[c][r][k] = sr_input_half<uint16_t, false>(v[c], 65535);
            }
        }
        const mfma_frag zero = {0u, 0u, 0u, 0u};
        if (a.unshuffle) {           // one pixel of the tensor: channel c 4 + r 2 + k
            uint16_t *o = a.out + (ptrdiff_t)b * SR_CIN0;
            *(mfma_frag *)__builtin_assume_aligned(o, 16) = mfma_frag{hv[0][0][0] | hv[0][0][1] << 16, hv[0][1][0] | hv[0][1][1] << 16,
                                                                      hv[1][0][0] | hv[1][0][1] << 16, hv[1][1][0] | hv[1][1][1] << 16};
            *(mfma_frag *)__builtin_assume_aligned(o + 8, 16) = mfma_frag{hv[2][0][0] | hv[2][0][1] << 16, hv[2][1][0] | hv[2][1][1] << 16, 0u, 0u};
            *(mfma_frag *)__builtin_assume_aligned(o + 16, 16) = zero;
            *(mfma_frag *)__builtin_assume_aligned(o + 24, 16) = zero;
            return;
        }
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int k = 0; k < 2; k++) {      // four pixels of the tensor: channels R, G, B
                uint16_t *o = a.out + ((ptrdiff_t)(2 * j + r) * a.sw + 2 * i + k) * SR_CIN0;
                *(mfma_frag *)__builtin_assume_aligned(o, 16) = mfma_frag{hv[0][r][k] | hv[1][r][k] << 16, hv[2][r][k], 0u, 0u};
#pragma unroll
                for (int q = 1; q < SR_CIN0 / 8; q++) *(mfma_frag *)__builtin_assume_aligned(o + q * 8, 16) = zero;
            }
    });
}

}  // namespace mihevc
