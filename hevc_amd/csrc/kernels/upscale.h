// hevc_amd/csrc/kernels/upscale.h — upscaling source (mihevc_send_frame_upscaled, mihevc_k_upscale_source): a planar 4:2:0 picture of sw x sh samples at 8 .. 16
// bit -> the session's own planar 4:2:0 planes of dw x dh (sw <= dw <= 4 sw, sh <= dh <= 4 sh) at 8 or 10 bit, margin included.  Separable Catmull-Rom
// interpolation, a blend towards the range of the two nearest samples after each pass (anti-ringing) and a limited 3x3 sharpener on luma, integers only, so that
// the device, the stepped kernel (tests/emu/upscale.cpp) and the numpy model (tests/upscale_ref.py) agree bit for bit.  The definition (normative: DESIGN.md
// §6k; the coefficient tables: csrc/scale_taps.h, scale_taps_build_up):
//   sample      the raw element r is a uint8 when B == 8, else a little-endian uint16; v = min(r, 2^B - 1)
//   tables      per axis of a plane, output sample i has near_i = floor(pos), a first source index f_i in near_i - 1 .. near_i + 2 and four coefficients
//               that sum to 4096 (zero padded): every non-zero one weighs a sample of near_i - 1 .. near_i + 2.  Source indices are clamped into the plane
//   blend       R(x, a, b) = x + ((clamp(x, min(a, b), max(a, b)) - x) ar + 4 >> 3), ar = 0 .. 8 eighths
//   horizontal  first: m = (sum_j c_j v[f_i + j] + 2^(11-G)) >> (12 - G), G = min(4, 16 - B) guard bits; m' = R(m, v[near_i] 2^G, v[near_i + 1] 2^G)
//   vertical    on m': t = (sum_j c_j m'[f_i + j] + 2^11) >> 12, t' = R(t, m'[near_i], m'[near_i + 1]), n = G + max(0, B - D) >= 1, u = max(0, D - B),
//               P = clamp((t' 2^u + 2^(n-1)) >> n, 0, 2^D - 1)                 (>>: arithmetic, rounds down)
//   sharpening  luma, gain g = 1 .. 64 sixteenths (0: off), on P inside the display area, neighbours clamped into it: c the sample, e the sum of its four edge
//               neighbours, f of its four corner neighbours; q = c + ((16 c - (4 c + 2 e + f)) g + 128 >> 8), out = clamp(q, min3x3, max3x3)
//   margin      as ingest.h: output sample (x, y) outside the display area equals the output sample at (min(x, dw - 1), min(y, dh - 1))
//   32 bits     sum |c_j| <= 5120 per row (scale_taps_build_up refuses otherwise): |sum c v| <= 5120 * 65535 < 2^29; |m|, |m'| <= 1.25 * 2^16; the blend's product
//               is below 2^21; |sum c m'| <= 5120 * 1.25 * 2^16 < 2^29; |t|, |t'| <= 1.5625 * 2^16, u > 0 only where B + G <= 13; |d16 g| <= 16 * 1023 * 64
// One launch per picture (k_upscale): a workgroup takes one tile of UP_TW x UP_TH output samples of one plane, the tiles of Y first, then Cb, then Cr.  A luma
// tile with g > 0 interpolates a halo of one output row and column around itself for the sharpener; image column q of a tile stands for output column
// clamp(x_base + q, 0, dw - 1) (rows alike), which gives the sharpener its clamped neighbours and the margin its copies.
//   phase 1   filters horizontally, with its blend, every source row the tile's output rows have a tap in (near - 1 of the first row .. near + 2 of the last:
//             at most UP_ROWS) into the LDS image m', 32 bits a sample (m overshoots 16 bits at B == 16).  A lane keeps one output column's coefficients
//             in registers and walks down the rows; the lanes of a wave take adjacent columns, whose source columns lie at most one apart: the four elements a
//             lane reads per row are the window near - 1 .. near + 2, the coefficients shifted to it, and the blend's two samples are its middle pair.  The raw
//             window is NOT staged in LDS: a wave's tap touches one or two cache lines and neighbouring lanes read the same elements, which the L1 serves.
//             Every global read is one element through ingest_element at a clamped column of a clamped row
//   phase 2   filters vertically out of m'.  Without a halo a lane produces ING_RUN adjacent samples of one row from two 16-byte LDS reads per row of the
//             window and stores them with one ingest_store; rows of m' are 528 bytes, so the rows of one ds_read_b128 group fall on alternate slots.  With the
//             halo the (UP_TH + 2) x (UP_TW + 2) samples P go into a second LDS image, 16 bits a sample
//   phase 3   (halo only) the sharpener out of the P image, a lane's run from three rows of ten samples, then ingest_store
// m' and P never reach HBM.
#pragma once
#include "ingest.h"

namespace mihevc {

constexpr int UP_LX = 16, UP_LY = NT / UP_LX;                 // lanes of the storing phase: 16 runs side by side x 16 rows
constexpr int UP_TW = UP_LX * ING_RUN, UP_TH = UP_LY;         // the tile: 128 x 16 output samples
constexpr int UP_HALO = 1;                                    // output rows / columns around a sharpened tile
constexpr int UP_COLS = UP_TW + 2 * UP_HALO, UP_PROWS = UP_TH + 2 * UP_HALO;
constexpr int UP_ROWS = UP_PROWS + 3;                         // source rows a tile can need: its rows' near spread over UP_PROWS - 1 at the most (1:1), + 4
constexpr int UP_MSTRIDE = 132, UP_PSTRIDE = 136;             // samples per image row: multiples of 16 bytes, and 4 banks off a multiple of 32

struct UpscaleShared {
    int32_t m[UP_ROWS][UP_MSTRIDE];         // 11,088 bytes
    uint16_t P[UP_PROWS][UP_PSTRIDE];       // 4,896 bytes
};

struct UpscaleArgs {
    const void *src[3];             // Y, Cb, Cr of the source
    void *dst[3];                   // coded-size planes; 16-byte aligned, strides too
    int pitch[3];                   // source, in elements
    int dstride[3];                 // in samples
    int sw, sh;                     // source size (luma)
    int dw, dh, pw, ph;             // display and coded size of the output (luma)
    const int32_t *first[4];        // tables: 0 luma horizontal, 1 luma vertical, 2 chroma horizontal, 3 chroma vertical; per output sample of the axis
    const int32_t *near[4];
    const int16_t *coef[4];         // four per output sample, rows 8-byte aligned
    int vmax;                       // v = min(r, vmax)
    int G, hround, hshift;          // m = (sum + hround) >> hshift; the blend's samples are v << G
    int n, u, peak;                 // P = clamp((t' << u) + (1 << (n - 1)) >> n, 0, peak)
    int ar, g;                      // antiring 0 .. 8, sharpen 0 .. 64
};

HDI bool upscale_geometry_ok(int sw, int sh, int dw, int dh)
{
    return sw >= 16 && sh >= 16 && dw >= 16 && dh >= 16 && !((sw | sh | dw | dh) & 1) && sw <= dw && dw <= 4 * sw && sh <= dh && dh <= 4 * sh;
}
HDI bool upscale_src_ok(const mihevc_upscale_src *f)
{
    if (!f || f->bit_depth < 8 || f->bit_depth > 16 || f->sharpen < 0 || f->sharpen > 64 || f->antiring < 0 || f->antiring > 8) return false;
    return !(f->reserved[0] | f->reserved[1] | f->reserved[2]);
}
HDI int upscale_tiles(int w, int h) { return ((w + UP_TW - 1) / UP_TW) * ((h + UP_TH - 1) / UP_TH); }
HDI int upscale_workgroups(int pw, int ph) { return upscale_tiles(pw, ph) + 2 * upscale_tiles(pw / 2, ph / 2); }
// workgroup r -> component (0 Y, 1 Cb, 2 Cr), r becomes the tile inside it; -1 past the last
HDI int upscale_locate(int pw, int ph, int &r)
{
    const int ny = upscale_tiles(pw, ph), nc = upscale_tiles(pw / 2, ph / 2);
    if (r < ny) return 0;
    r -= ny;
    if (r < nc) return 1;
    r -= nc;
    return r < nc ? 2 : -1;
}
// every field from the source, the geometry, the planes and the tables (first / near / coef as UpscaleArgs: where the kernel will read them)
inline UpscaleArgs upscale_args(const mihevc_upscale_src &f, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int dw, int dh, int pw, int ph,
                                int out_depth, void *const *out, const int *ostride, const int32_t *const *first, const int32_t *const *near, const int16_t *const *coef)
{
    UpscaleArgs a;
    const int B = f.bit_depth;
    a.src[0] = y; a.src[1] = u; a.src[2] = v;
    for (int c = 0; c < 3; c++) { a.dst[c] = out[c]; a.dstride[c] = ostride[c]; a.pitch[c] = c ? pitch_c : pitch_y; }
    for (int k = 0; k < 4; k++) { a.first[k] = first[k]; a.near[k] = near[k]; a.coef[k] = coef[k]; }
    a.sw = f.width; a.sh = f.height; a.dw = dw; a.dh = dh; a.pw = pw; a.ph = ph;
    a.G = 16 - B < 4 ? 16 - B : 4;
    a.vmax = (1 << B) - 1;
    a.hshift = 12 - a.G; a.hround = 1 << (11 - a.G);
    a.n = a.G + (B > out_depth ? B - out_depth : 0); a.u = out_depth > B ? out_depth - B : 0; a.peak = (1 << out_depth) - 1;
    a.ar = f.antiring; a.g = f.sharpen;
    return a;
}

// x, `ar` eighths of the way into the range of a and b
DEV int upscale_blend(int x, int a, int b, int ar) { return x + (((clip3(imin(a, b), imax(a, b), x) - x) * ar + 4) >> 3); }
// near of output sample i and its four coefficients shifted to the window near - 1 .. near + 2 (first - near + 1 is 0 .. 3: scale_taps_build_up)
DEV int upscale_coefs(const int32_t *first, const int32_t *near, const int16_t *coef, int i, int (&c)[4])
{
    const ingest_u32x2 raw = *(const ingest_u32x2 *)__builtin_assume_aligned(coef + (ptrdiff_t)i * 4, 8);
    const int nr = near[i];
    const uint64_t w = ((uint64_t)raw[1] << 32 | raw[0]) << (16 * ((first[i] - nr + 1) & 3));
#pragma unroll
    for (int j = 0; j < 4; j++) c[j] = (int)(int16_t)(w >> (16 * j));
    return nr;
}
typedef int32_t upscale_i32x4 __attribute__((vector_size(16), may_alias));

// workgroup `wg` of the launch
template <typename TI, typename TO, class Ex> DEV void upscale_tile_program(Ex &ex, UpscaleShared &s, const UpscaleArgs &a, int wg)
{
    int tile = wg;
    const int c = upscale_locate(a.pw, a.ph, tile);
    if (c < 0) return;
    // Every field is read here, once: the phases below read none (reads of `a` behind ingest_element's compiler barrier keep the kernel's
    // private copy of the argument block alive, in scratch)
    const int th = c ? 2 : 0, tv = th + 1;                                                              // the plane's tables
    const int32_t *const first_h = a.first[th], *const first_v = a.first[tv], *const near_h = a.near[th], *const near_v = a.near[tv];
    const int16_t *const coef_h = a.coef[th], *const coef_v = a.coef[tv];
    const TI *const src = (const TI *)a.src[c];
    TO *const dst = (TO *)a.dst[c];
    const int pitch_c = a.pitch[c], dstride_c = a.dstride[c];
    const int vmax = a.vmax, G = a.G, hround = a.hround, hshift = a.hshift, peak = a.peak, up = 1 << a.u, n = a.n, ar = a.ar;
    const int g = c ? 0 : a.g, halo = g > 0 ? UP_HALO : 0;                                              // uniform: the sharpened tiles carry the halo
    const int ssw = c ? a.sw / 2 : a.sw, ssh = c ? a.sh / 2 : a.sh;                                     // source plane
    const int dwo = c ? a.dw / 2 : a.dw, dho = c ? a.dh / 2 : a.dh, pwo = c ? a.pw / 2 : a.pw, pho = c ? a.ph / 2 : a.ph;
    const int ntx = (pwo + UP_TW - 1) / UP_TW, ty = tile / ntx, tx = tile - ty * ntx;
    const int x_base = tx * UP_TW - halo, y_base = ty * UP_TH - halo;                                   // output sample of image column / row 0, before clamping
    const int k0 = near_v[clip3(0, dho - 1, y_base)] - 1;                                               // source row of row 0 of m' (before clamping)
    const int nrows = imin(near_v[clip3(0, dho - 1, y_base + UP_TH + 2 * halo - 1)] + 3 - k0, UP_ROWS);      // .. near + 2 of the last row
    ex.phase([&](int tid) {          // horizontal.  Pass 0: column tid % UP_TW of rows tid / UP_TW, + 2, ...; pass 1: the two columns of the halo
        for (int pass = 0; pass <= halo; pass++) {
            const int q = pass ? UP_TW + (tid & 1) : tid & (UP_TW - 1), step = pass ? NT / 2 : NT / UP_TW;
            int cf[4];
            const int nr = upscale_coefs(first_h, near_h, coef_h, clip3(0, dwo - 1, x_base + q), cf);
            const int x0 = clip3(0, ssw - 1, nr - 1), x1 = clip3(0, ssw - 1, nr), x2 = clip3(0, ssw - 1, nr + 1), x3 = clip3(0, ssw - 1, nr + 2);
            for (int l = pass ? tid >> 1 : tid / UP_TW; l < nrows; l += step) {
                const TI *row = src + (ptrdiff_t)clip3(0, ssh - 1, k0 + l) * pitch_c;
                int v0, v1, v2, v3;      // every load of the row first
                ingest_element(row + x0, v0);
                ingest_element(row + x1, v1);
                ingest_element(row + x2, v2);
                ingest_element(row + x3, v3);
                v0 = imin(v0, vmax); v1 = imin(v1, vmax); v2 = imin(v2, vmax); v3 = imin(v3, vmax);
                const int m = (cf[0] * v0 + cf[1] * v1 + cf[2] * v2 + cf[3] * v3 + hround) >> hshift;
                s.m[l][q] = upscale_blend(m, v1 << G, v2 << G, ar);
            }
        }
    });
    // one sample of P: column q of m', rows l .. l + 3
    auto vertical = [&](const int (&cf)[4], int m0, int m1, int m2, int m3) {
        const int t = (cf[0] * m0 + cf[1] * m1 + cf[2] * m2 + cf[3] * m3 + (1 << 11)) >> 12;
        return clip3(0, peak, (upscale_blend(t, m1, m2, ar) * up + (1 << (n - 1))) >> n);
    };
    if (!halo) {
        ex.phase([&](int tid) {      // vertical: the lane's run of ING_RUN samples, stored
            const int lx = tid & (UP_LX - 1), ly = tid / UP_LX, cx = lx * ING_RUN, x0 = tx * UP_TW + cx, y = ty * UP_TH + ly;
            if (x0 >= pwo || y >= pho) return;
            int cf[4];
            const int l = clip3(0, UP_ROWS - 4, upscale_coefs(first_v, near_v, coef_v, imin(y, dho - 1), cf) - 1 - k0);      // 0 <= l, l + 3 < nrows; the clip only guards the image
            upscale_i32x4 r[4][2];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int32_t *p = &s.m[l + j][cx];
                r[j][0] = *(const upscale_i32x4 *)__builtin_assume_aligned(p, 16); r[j][1] = *(const upscale_i32x4 *)__builtin_assume_aligned(p + 4, 16);
            }
            int o[ING_RUN];
#pragma unroll
            for (int k = 0; k < ING_RUN; k++) o[k] = vertical(cf, r[0][k >> 2][k & 3], r[1][k >> 2][k & 3], r[2][k >> 2][k & 3], r[3][k >> 2][k & 3]);
            ingest_store(dst + (ptrdiff_t)y * dstride_c + x0, o, x0 + ING_RUN <= pwo);
        });
        return;
    }
    ex.phase([&](int tid) {          // vertical into the P image.  Pass 0: column tid % UP_TW of rows tid / UP_TW, + 2, ...; pass 1: the two columns of the halo
        for (int pass = 0; pass < 2; pass++) {
            const int q = pass ? UP_TW + (tid & 1) : tid & (UP_TW - 1), step = pass ? NT / 2 : NT / UP_TW;
            for (int r = pass ? tid >> 1 : tid / UP_TW; r < UP_PROWS; r += step) {
                int cf[4];
                const int l = clip3(0, UP_ROWS - 4, upscale_coefs(first_v, near_v, coef_v, clip3(0, dho - 1, y_base + r), cf) - 1 - k0);
                s.P[r][q] = (uint16_t)vertical(cf, s.m[l][q], s.m[l + 1][q], s.m[l + 2][q], s.m[l + 3][q]);
            }
        }
    });
    ex.phase([&](int tid) {          // the sharpener: the lane's run out of three rows of ten samples of P
        const int lx = tid & (UP_LX - 1), ly = tid / UP_LX, cx = lx * ING_RUN, x0 = tx * UP_TW + cx, y = ty * UP_TH + ly;
        if (x0 >= pwo || y >= pho) return;
        const int rc = imin(y, dho - 1) - y_base;           // image row of the sample (of the last display row for a row of the margin): 1 .. UP_TH
        int w[3][ING_RUN + 2];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const uint16_t *p = &s.P[rc - 1 + j][cx];       // image columns cx .. cx + 9: output columns x0 - 1 .. x0 + 8, clamped into the display area
            const ingest_u32x4 lo = *(const ingest_u32x4 *)__builtin_assume_aligned(p, 16);
            const uint32_t hi = load_u32_aligned(p + 8);
#pragma unroll
            for (int k = 0; k < 8; k++) w[j][k] = (int)((lo[k >> 1] >> (16 * (k & 1))) & 0xffffu);
            w[j][8] = (int)(hi & 0xffffu); w[j][9] = (int)(hi >> 16);
        }
        int o[ING_RUN];
#pragma unroll
        for (int k = 0; k < ING_RUN; k++) {
            const int ctr = w[1][k + 1], e = w[0][k + 1] + w[2][k + 1] + w[1][k] + w[1][k + 2], f = w[0][k] + w[0][k + 2] + w[2][k] + w[2][k + 2];
            int lo = ctr, hi = ctr;
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int i = 0; i < 3; i++) { lo = imin(lo, w[j][k + i]); hi = imax(hi, w[j][k + i]); }
            o[k] = clip3(lo, hi, ctr + (((16 * ctr - (4 * ctr + 2 * e + f)) * g + 128) >> 8));
            if (k && x0 + k > dwo - 1) o[k] = o[k - 1];     // the margin repeats the last display column (a run begins inside the display area: pw - dw < ING_RUN)
        }
        ingest_store(dst + (ptrdiff_t)y * dstride_c + x0, o, x0 + ING_RUN <= pwo);
    });
}

}  // namespace mihevc
