// hevc_amd/csrc/kernels/ingest_rgb.h — RGB sources (mihevc_send_frame_rgb, mihevc_k_convert_rgb): a full-range R'G'B' picture, planar or packed, 8 .. 16 bit
// integers or IEEE half / single floats -> the session's planar 4:2:0 Y'CbCr planes at 8 or 10 bit, limited or full range, margin included: colour matrix, range
// scale, chroma filter and decimation in one pass.  Integers only behind the sample rule, so that the device, the stepped kernel (tests/emu/ingest_rgb.cpp) and
// the numpy model (tests/ingest_rgb_ref.py) agree bit for bit.  The definition (normative; DESIGN.md 6d repeats it):
//   picture  W x H (display size, both even).  B = significant bits of a source sample (8 .. 16), lsb aligned; D = the session's bit depth (8 or 10)
//   sample   integers: the raw element r is a uint8 when B == 8, else a little-endian uint16; v = min(r, 2^B - 1).
//            floats (planar only; a half is widened to float32 exactly first, so subnormal halves count): B = 16 and v = rint(min(max(x, 0), 1) * 65535): one
//            float32 multiplication rounded to nearest even, rint ties-to-even, NaN -> 0.  No fast-math and no contraction on this path
//   matrix   code 1 (BT.709), 5 or 6 (BT.601), 9 (BT.2020 ncl): (Kr, Kb) in 1/10000 = (2126, 722), (2990, 1140), (2627, 593); Kg = 1 - Kr - Kb.
//            rows  Y (Kr, Kg, Kb);  Cb (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb));  Cr (1 - Kr, -Kg, -Kb) / (2 (1 - Kr))
//   scale    limited: sY = 219 2^(D-8) / (2^B - 1), sC = 224 2^(D-8) / (2^B - 1), oY = 16 2^(D-8); full: sY = sC = (2^D - 1) / (2^B - 1), oY = 0; oC = 2^(D-1)
//   coefficients  S = 16 + max(0, B - D); m[r][c] = floor(row[r][c] s 2^S + 1/2) evaluated exactly (ingest_rgb_matrix: integers, no doubles)
//   pixel    t[r] = m[r][0] R + m[r][1] G + m[r][2] B in 64 bits (at B = 16 the sums pass 2^31)
//   luma     Y = clip(((t[0] + 2^(S-1)) >> S) + oY, 0, 2^D - 1)
//   chroma   the siting and taps of the 4:4:4 path of ingest.h: for output (i, j), T = sum over rows {2j, 2j+1} of t[c] at column max(2i-1, 0) + 2 t[c] at
//            column 2i + t[c] at column 2i+1; C = clip(((T + 2^(S+2)) >> (S+3)) + oC, 0, 2^D - 1).  Shifts of negative values are arithmetic (floor); one
//            rounding, after the filter
//   margin   as ingest.h: output sample (x, y) outside the display area equals the output sample at (min(x, sw - 1), min(y, sh - 1))
// One launch per picture (k_ingest_rgb), no LDS.  A lane owns a block of RGB_BW x 2 source pixels: it reads them once, writes two luma runs per row and one run of
// Cb and of Cr (the last block of a row may be half a block: coded widths are multiples of 8); the only re-read is the pixel left of the block, the clamped
// left tap.  The components' places (which plane, which element of a packed pixel) are folded into the columns of the matrix on the host, so the kernel does not
// know an order; an unused fourth element meets a zero coefficient.  A block inside the display area reads its rows in chunks of 16, 8 or 4 bytes, the widest
// that the base addresses and the pitch allow (IngestRgbArgs::align: a uniform branch), or element by element; a block that reaches into the margin, and the left
// tap, read single elements at clamped coordinates.  A block of a packed row is RGB_BW x 3 or x 4 elements: a multiple of 16 bytes for every element type, so
// 3-byte pixels take the same chunks as everything else and a pixel may straddle two of them.  The chunk loads, the element load and the stores are those of
// ingest.h (ingest_load, ingest_element, ingest_store), behind its one access hook.
#pragma once
#include "ingest.h"

namespace mihevc {

constexpr int RGB_BW = 2 * ING_RUN;                 // source columns per lane (two rows of them)
constexpr int RGB_LX = 16, RGB_LY = NT / RGB_LX;    // lanes of a workgroup: 16 blocks side by side x 16 block rows
constexpr int RGB_TW = RGB_LX * RGB_BW, RGB_TH = 2 * RGB_LY;

struct IngestRgbArgs {
    const void *src[3];      // three planes, or the packed plane in src[0]
    void *dst[3];            // coded-size planes; 16-byte aligned, strides too
    int dstride[3];          // in samples
    int pitch;               // source, in elements, every plane
    int align;               // 16, 8, 4 or 1: what every source plane allows (ingest_align)
    int sw, sh, pw, ph;      // display and coded size of luma
    int epp;                 // elements per pixel in a row: 1 (planes), 3, 4
    int vmax;                // integer samples: v = min(r, vmax)
    int m[3][4];             // m[row][e]: the coefficient that meets plane e / element e of a pixel; 0 where no component sits
    int S, oY, oC, peak;
};

HDI bool rgb_format_ok(const mihevc_rgb_format *f)
{
    if (!f || (f->layout != 0 && f->layout != 3 && f->layout != 4)) return false;
    const int n = f->layout ? f->layout : 3;
    if (f->r < 0 || f->r >= n || f->g < 0 || f->g >= n || f->b < 0 || f->b >= n || f->r == f->g || f->r == f->b || f->g == f->b) return false;
    if (f->sample < 0 || f->sample > 2 || (f->sample && (f->layout || f->bit_depth)) || (!f->sample && (f->bit_depth < 8 || f->bit_depth > 16))) return false;
    if ((f->matrix != 0 && f->matrix != 1 && f->matrix != 5 && f->matrix != 6 && f->matrix != 9) || f->range < 0 || f->range > 2) return false;
    return !(f->reserved[0] | f->reserved[1] | f->reserved[2] | f->reserved[3]);
}
HDI bool rgb_matrix_ok(int matrix) { return matrix == 1 || matrix == 5 || matrix == 6 || matrix == 9; }
HDI int rgb_elem_size(const mihevc_rgb_format &f) { return f.sample == 2 ? 4 : f.sample == 1 || f.bit_depth > 8 ? 2 : 1; }
HDI int rgb_row_elems(const mihevc_rgb_format &f, int w) { return f.layout ? f.layout * w : w; }
HDI int rgb_planes(const mihevc_rgb_format &f) { return f.layout ? 1 : 3; }
// the planes the layout needs are there and aligned to their element, and the pitch (elements) holds a row of `w` pixels
HDI bool rgb_planes_ok(const mihevc_rgb_format &f, const void *const *p, int pitch, int w)
{
    for (int c = 0; c < rgb_planes(f); c++)
        if (!p[c] || (uintptr_t)p[c] % (unsigned)rgb_elem_size(f)) return false;
    return pitch >= rgb_row_elems(f, w);
}
HDI int ingest_rgb_workgroups(int pw, int ph) { return ((pw + RGB_TW - 1) / RGB_TW) * ((ph + RGB_TH - 1) / RGB_TH); }

inline int64_t rgb_floor_div(int64_t a, int64_t b)      // b > 0
{
    const int64_t q = a / b;
    return a % b < 0 ? q - 1 : q;
}
// m[r][c] = floor(row[r][c] s 2^S + 1/2) for R, G, B in this order, exactly: every factor is a ratio of integers.  B, D: sample and session depth
inline bool ingest_rgb_matrix(int matrix, bool full, int B, int D, int (&m)[3][3], int &S)
{
    int64_t kr, kb;
    if (matrix == 1) { kr = 2126; kb = 722; }
    else if (matrix == 5 || matrix == 6) { kr = 2990; kb = 1140; }
    else if (matrix == 9) { kr = 2627; kb = 593; }
    else return false;
    const int64_t kg = 10000 - kr - kb, peak = ((int64_t)1 << D) - 1, unit = (int64_t)1 << (D - 8);
    S = 16 + (B > D ? B - D : 0);
    const int64_t num[3][3] = {{kr, kg, kb}, {-kr, -kg, 10000 - kb}, {10000 - kr, -kg, -kb}};
    const int64_t den[3] = {10000, 2 * (10000 - kb), 2 * (10000 - kr)};
    const int64_t s_num[3] = {full ? peak : 219 * unit, full ? peak : 224 * unit, full ? peak : 224 * unit}, s_den = ((int64_t)1 << B) - 1;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const int64_t P = num[r][c] * s_num[r] * ((int64_t)1 << S), Q = den[r] * s_den;      // |P| < 2^48, Q < 2^32
            m[r][c] = (int)rgb_floor_div(2 * P + Q, 2 * Q);
        }
    return true;
}
// every field from the format (matrix and range resolved by the caller), the geometry and the planes
inline IngestRgbArgs ingest_rgb_args(const mihevc_rgb_format &f, int matrix, bool full, const void *p0, const void *p1, const void *p2, int pitch, int sw, int sh,
                                     int pw, int ph, int out_depth, void *const *out, const int *ostride)
{
    IngestRgbArgs a;
    const int B = f.sample ? 16 : f.bit_depth, planes = rgb_planes(f);
    a.src[0] = p0; a.src[1] = planes == 3 ? p1 : nullptr; a.src[2] = planes == 3 ? p2 : nullptr;
    a.pitch = pitch; a.align = 16;
    for (int c = 0; c < 3; c++) {
        a.dst[c] = out[c]; a.dstride[c] = ostride[c];
        if (c < planes) {
            const int al = ingest_align(a.src[c], (size_t)pitch * rgb_elem_size(f));
            if (al < a.align) a.align = al;
        }
    }
    a.sw = sw; a.sh = sh; a.pw = pw; a.ph = ph; a.epp = f.layout ? f.layout : 1; a.vmax = (1 << B) - 1;
    int m[3][3];
    ingest_rgb_matrix(matrix, full, B, out_depth, m, a.S);
    for (int r = 0; r < 3; r++) {
        for (int e = 0; e < 4; e++) a.m[r][e] = 0;
        a.m[r][f.r] = m[r][0]; a.m[r][f.g] = m[r][1]; a.m[r][f.b] = m[r][2];
    }
    a.oY = full ? 0 : 16 << (out_depth - 8); a.oC = 1 << (out_depth - 1); a.peak = (1 << out_depth) - 1;
    return a;
}

// ---- the float rule.  No contraction can arise: the one product feeds rint, not a sum
DEV float rgb_float_of_bits(uint32_t b)
{
    float f;
    __builtin_memcpy(&f, &b, 4);
    return f;
}
// exact: a half's 11 significant bits and its exponents -24 .. 15 all fit a float32; a subnormal half is its integer mantissa times 2^-24
DEV float rgb_float_of_half(uint32_t h)
{
    const uint32_t e = (h >> 10) & 31u, m = h & 1023u;
    const float mag = e == 0 ? (float)(int)m * 0x1p-24f : rgb_float_of_bits(e == 31 ? 0x7f800000u | m << 13 : (e + 112u) << 23 | m << 13);
    return (h & 0x8000u) ? -mag : mag;
}
DEV int rgb_unit_to_16(float x)
{
    x = x > 0.0f ? x : 0.0f;      // NaN compares false: 0
    x = x < 1.0f ? x : 1.0f;
    return (int)__builtin_rintf(x * 65535.0f);
}
// the sample value of a raw element.  TI: uint8_t / uint16_t integers, or with FLT uint16_t (half) / uint32_t (single)
template <typename TI, bool FLT> DEV int rgb_value(int raw, int vmax)
{
    if constexpr (!FLT) return imin(raw, vmax);
    else if constexpr (sizeof(TI) == 2) return rgb_unit_to_16(rgb_float_of_half((uint32_t)raw));
    else return rgb_unit_to_16(rgb_float_of_bits((uint32_t)raw));
}

// ---- one pixel
struct RgbT { int64_t y, cb, cr; };
// E values of a pixel's planes / elements -> t[0 .. 2]
template <int E> DEV RgbT rgb_matrix(const IngestRgbArgs &a, const int (&e)[E])
{
    int64_t t[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        t[r] = 0;
#pragma unroll
        for (int k = 0; k < E; k++) t[r] += (int64_t)a.m[r][k] * e[k];
    }
    return RgbT{t[0], t[1], t[2]};
}
// the pixel of column x of a row, element by element.  row[c]: the first element of the row in plane c (a packed source: row[0] only)
template <typename TI, bool FLT, int EPP> DEV RgbT rgb_pixel_at(const IngestRgbArgs &a, const TI *const (&row)[3], int x)
{
    constexpr int E = EPP == 1 ? 3 : EPP;
    int e[E];
#pragma unroll
    for (int k = 0; k < E; k++) {
        ingest_element(EPP == 1 ? row[k] + x : row[0] + (ptrdiff_t)x * EPP + k, e[k]);
        e[k] = rgb_value<TI, FLT>(e[k], a.vmax);
    }
    return rgb_matrix<E>(a, e);
}
DEV int rgb_luma(const IngestRgbArgs &a, int64_t t) { return imax(imin((int)((t + ((int64_t)1 << (a.S - 1))) >> a.S) + a.oY, a.peak), 0); }
DEV int rgb_chroma(const IngestRgbArgs &a, int64_t T) { return imax(imin((int)((T + ((int64_t)1 << (a.S + 2))) >> (a.S + 3)) + a.oC, a.peak), 0); }

// One source row of a block: Y[k]: the luma of output column x0 + k; T[c][k] += the row's share of chroma output x0 / 2 + k.  y: the source row;
// cols: the chroma columns of the block that are stored (half a block at the right edge: ING_RUN / 2), the others are not worked out
template <typename TI, bool FLT, int EPP> DEV void rgb_row(const IngestRgbArgs &a, int y, int x0, int cols, int (&Y)[RGB_BW], int64_t (&T)[2][ING_RUN])
{
    constexpr int E = EPP == 1 ? 3 : EPP;
    const TI *row[3];
#pragma unroll
    for (int c = 0; c < 3; c++) row[c] = (const TI *)a.src[EPP == 1 ? c : 0] + (ptrdiff_t)y * a.pitch;
    if (x0 + RGB_BW <= a.sw) {           // the whole block lies in the display area
        int v[EPP == 1 ? 3 : 1][RGB_BW * EPP];
#pragma unroll
        for (int c = 0; c < (EPP == 1 ? 3 : 1); c++) {
            static_assert(RGB_BW * EPP * sizeof(TI) % 16 == 0, "a block of a row is a whole number of 16-byte chunks");
            ingest_load<TI, RGB_BW * EPP>(row[c] + (ptrdiff_t)x0 * EPP, a.align, v[c]);
#pragma unroll
            for (int i = 0; i < RGB_BW * EPP; i++) v[c][i] = rgb_value<TI, FLT>(v[c][i], a.vmax);
        }
        RgbT left = rgb_pixel_at<TI, FLT, EPP>(a, row, imax(x0 - 1, 0));
#pragma unroll
        for (int k = 0; k < ING_RUN; k++) {
            RgbT t[2];
#pragma unroll
            for (int q = 0; q < 2; q++) {
                int e[E];
#pragma unroll
                for (int j = 0; j < E; j++) {
                    if constexpr (EPP == 1) e[j] = v[j][2 * k + q];
                    else e[j] = v[0][(2 * k + q) * EPP + j];
                }
                t[q] = rgb_matrix<E>(a, e);
                Y[2 * k + q] = rgb_luma(a, t[q].y);
            }
            T[0][k] += left.cb + 2 * t[0].cb + t[1].cb;
            T[1][k] += left.cr + 2 * t[0].cr + t[1].cr;
            left = t[1];
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < RGB_BW; k++) Y[k] = 0;
#pragma unroll 1
    for (int k = 0; k < cols; k++) {         // the block reaches into the margin: chroma columns clamped to the display area, one element at a time
        const int i = imin(x0 / 2 + k, a.sw / 2 - 1);
        const RgbT l = rgb_pixel_at<TI, FLT, EPP>(a, row, imax(2 * i - 1, 0)), t0 = rgb_pixel_at<TI, FLT, EPP>(a, row, 2 * i), t1 = rgb_pixel_at<TI, FLT, EPP>(a, row, 2 * i + 1);
        const int y1 = rgb_luma(a, t1.y), y0 = x0 / 2 + k == i ? rgb_luma(a, t0.y) : y1;      // past the display area both columns repeat the last one
#pragma unroll
        for (int j = 0; j < ING_RUN; j++)        // (no indexing of registers by k)
            if (j == k) { Y[2 * j] = y0; Y[2 * j + 1] = y1; T[0][j] += l.cb + 2 * t0.cb + t1.cb; T[1][j] += l.cr + 2 * t0.cr + t1.cr; }
    }
}

// the lane's block of tile `tile`: luma rows 2j and 2j + 1, chroma row j
template <typename TI, bool FLT, typename TO, int EPP> DEV void rgb_block(const IngestRgbArgs &a, int tile, int tid)
{
    const int ntx = (a.pw + RGB_TW - 1) / RGB_TW, ty = tile / ntx, tx = tile - ty * ntx;
    const int x0 = (tx * RGB_LX + (tid & (RGB_LX - 1))) * RGB_BW, j = ty * RGB_LY + tid / RGB_LX;
    if (x0 >= a.pw || 2 * j >= a.ph) return;
    const bool inside = j < a.sh / 2, wide = x0 + RGB_BW <= a.pw;      // below the display area the block reads the last two rows; wide: both runs of a luma row
    const int js = inside ? j : a.sh / 2 - 1;
    int64_t T[2][ING_RUN];
#pragma unroll
    for (int k = 0; k < ING_RUN; k++) T[0][k] = T[1][k] = 0;
    auto store_luma = [&](int y, const int (&Y)[RGB_BW]) {
        TO *p = (TO *)a.dst[0] + (ptrdiff_t)y * a.dstride[0] + x0;
        int o[ING_RUN];
#pragma unroll
        for (int k = 0; k < ING_RUN; k++) o[k] = Y[k];
        ingest_store(p, o, true);
        if (!wide) return;
#pragma unroll
        for (int k = 0; k < ING_RUN; k++) o[k] = Y[ING_RUN + k];
        ingest_store(p + ING_RUN, o, true);
    };
#pragma unroll 1
    for (int r = 0; r < 2; r++) {
        int Y[RGB_BW];
        rgb_row<TI, FLT, EPP>(a, 2 * js + r, x0, wide ? ING_RUN : ING_RUN / 2, Y, T);
        if (r || inside) store_luma(2 * j + r, Y);
        if (r && !inside) store_luma(2 * j, Y);      // both luma rows repeat the last source row
    }
#pragma unroll
    for (int c = 0; c < 2; c++) {
        int o[ING_RUN];
#pragma unroll
        for (int k = 0; k < ING_RUN; k++) o[k] = rgb_chroma(a, T[c][k]);
        ingest_store((TO *)a.dst[1 + c] + (ptrdiff_t)j * a.dstride[1 + c] + x0 / 2, o, wide);
    }
}

// workgroup `wg` of the launch
template <typename TI, bool FLT, typename TO, class Ex> DEV void ingest_rgb_tile_program(Ex &ex, const IngestRgbArgs &a, int wg)
{
    if (wg >= ingest_rgb_workgroups(a.pw, a.ph)) return;
    ex.phase([&](int tid) {
        if constexpr (FLT) rgb_block<TI, FLT, TO, 1>(a, wg, tid);
        else if (a.epp == 1) rgb_block<TI, FLT, TO, 1>(a, wg, tid);
        else if (a.epp == 3) rgb_block<TI, FLT, TO, 3>(a, wg, tid);
        else rgb_block<TI, FLT, TO, 4>(a, wg, tid);
    });
}

}  // namespace mihevc
