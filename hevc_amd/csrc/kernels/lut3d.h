// hevc_amd/csrc/kernels/lut3d.h — colour through a 3D lookup table (mihevc_set_lut3d, mihevc_send_frame_lut3d, mihevc_k_lut3d): a planar 4:2:0 Y'CbCr picture at
// 8, 10 or 12 bit -> R'G'B' at 16 bit -> an N x N x N table with tetrahedral interpolation -> the session's planar 4:2:0 planes at 8 or 10 bit with the session's own
// matrix and range, margin included: HDR to SDR, log to Rec.709 or any grade shipped as a .cube file, in one launch.  Integers only, so that the device, the
// stepped kernel (tests/emu/lut3d.cpp) and the numpy model (tests/lut3d_ref.py) agree bit for bit.  The definition (normative; DESIGN.md 6i repeats it).  Shifts of
// negative values are arithmetic:
//   picture  W x H (display size, both even), source planar 4:2:0.  B = 8, 10 or 12; elements uint8 at B = 8, else little-endian uint16, lsb aligned,
//            v = min(r, 2^B - 1).  Source matrix code 1, 5, 6 or 9, source range limited or full.  D = the session's bit depth (8 or 10)
//   1 chroma to the luma grid (the siting 6c / 6d filter down to: co-sited with even columns, centred between rows 2j and 2j+1), no rounding, factor 8:
//            h(i, 2x) = 2 c[i][x], h(i, 2x+1) = c[i][x] + c[i][min(x+1, W/2-1)];
//            row 2j: C8 = 3 h(j, .) + h(max(j-1, 0), .); row 2j+1: C8 = 3 h(j, .) + h(min(j+1, H/2-1), .)
//   2 Y'CbCr -> R'G'B' at 16 bit: y = Y - oY, cb = Cb8 - 8 oC, cr = Cr8 - 8 oC; oY = 16 2^(B-8) (full: 0), oC = 2^(B-1).  With (Kr, Kb) as in 6d, Kg = 1 - Kr - Kb,
//            limited sY = 65535 / (219 2^(B-8)), sC = 65535 / (224 2^(B-8)); full sY = sC = 65535 / (2^B - 1), the five coefficients
//              nY = sY;  nRv = 2 (1 - Kr) sC / 8;  nGu = -(2 Kb (1 - Kb) / Kg) sC / 8;  nGv = -(2 Kr (1 - Kr) / Kg) sC / 8;  nBu = 2 (1 - Kb) sC / 8
//            (the 1/8 that undoes the factor of step 1 is part of the coefficient) are n = floor(coef 2^16 + 1/2), evaluated exactly (lut3d_inverse: integers, no
//            doubles).  t_R = nY y + nRv cr, t_G = nY y + nGu cb + nGv cr, t_B = nY y + nBu cb in 64 bits; v = clip((t + 2^15) >> 16, 0, 65535)
//   3 table  N points per axis, 2 <= N <= 65, uint16 triples L[b][g][r][c] (red fastest: the order of a .cube file).  Per component p = v (N - 1),
//            i = min(p / 65535, N - 2), f = p - 65535 i (0 .. 65535; 65535 only at v = 65535).  Fractions sorted f1 >= f2 >= f3 with their axes a1, a2, a3;
//            V0 = L at (i_r, i_g, i_b), V1 = V0 stepped along a1, V2 = V1 stepped along a2, V3 = V0 stepped along all three;
//            o_c = ((65535 - f1) V0_c + (f1 - f2) V1_c + (f2 - f3) V2_c + f3 V3_c + 32767) / 65535 (integer division; the dividend is below 2^32).  Equal
//            fractions may be ordered either way: the vertex they disagree on has weight 0
//   4 R'G'B' -> the session's planes: from "matrix" on, 6d (ingest_rgb.h) unchanged with B = 16: coefficients, luma, the (1 2 1) x 2-row chroma filter with its one
//            rounding, clipping, margin
// One launch per picture (k_lut3d), no LDS.  The work is cut as k_ingest_rgb cuts it: a lane owns a block of RGB_BW x 2 pixels, reads their luma and the chroma rows
// around them once, writes two luma runs per row and one run of Cb and of Cr; the pixel left of the block (the clamped left tap of step 4) is evaluated again, element
// by element, which costs four more table vertices per block row.  The table arrives repacked into 8-byte entries (R, G, B, pad), so a vertex is one 8-byte load
// and a pixel takes four; at N = 65 the table is 2.2 MB, at N = 33 0.29 MB: both stay in an XCD's L2.  The two divisions by 65535 are a multiply-free shift form
// (lut_div65535) that is exact below 65535 * 65536 (tests/emu/lut3d.cpp checks every boundary).  The pixel function (lut_rgb16, lut_lookup) knows nothing of the
// source's layout.  Step 4, the loads, the element load and the stores are those of ingest_rgb.h and ingest.h, behind ingest.h's one access hook.
#pragma once
#include "ingest_rgb.h"

namespace mihevc {

constexpr int LUT_MIN_N = 2, LUT_MAX_N = 65;
constexpr int LUT_ENTRY_BYTES = 8;      // a packed table entry: R, G, B, pad as four uint16

struct Lut3dArgs {
    IngestRgbArgs out;       // step 4 and the geometry: three "planes" R, G, B at 16 bit in registers (out.src is unused)
    const void *src[3];      // Y, Cb, Cr
    int pitch[3];            // in elements
    int align[3];            // per source plane: 16, 8, 4 or 1 (ingest_align)
    const void *table;       // n^3 packed entries, 8-byte aligned
    int n;
    int vmax, oY, oC8;       // v = min(r, vmax); y = Y - oY; cb = Cb8 - oC8
    int nY, nRv, nGu, nGv, nBu;
};

HDI bool lut3d_n_ok(int n) { return n >= LUT_MIN_N && n <= LUT_MAX_N; }
HDI bool lut3d_src_ok(const mihevc_lut3d_src *f)
{
    if (!f || (f->bit_depth != 8 && f->bit_depth != 10 && f->bit_depth != 12) || !rgb_matrix_ok(f->matrix) || (f->full_range != 0 && f->full_range != 1)) return false;
    return !(f->reserved[0] | f->reserved[1] | f->reserved[2] | f->reserved[3]);
}
// the planes are there and aligned to their element, and the pitches (elements) hold a row of `w` luma samples
HDI bool lut3d_planes_ok(const mihevc_lut3d_src &f, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int w)
{
    const unsigned es = f.bit_depth > 8 ? 2 : 1;
    if (!y || !u || !v || (uintptr_t)y % es || (uintptr_t)u % es || (uintptr_t)v % es) return false;
    return pitch_y >= w && pitch_c >= w / 2;
}
// the table of a .cube file, n^3 x 3 uint16 with red fastest, as the kernel reads it: n^3 entries of four uint16 (R, G, B, 0)
inline void lut3d_pack(int n, const uint16_t *table, uint16_t *packed)
{
    for (size_t i = 0; i < (size_t)n * n * n; i++) {
        packed[4 * i] = table[3 * i]; packed[4 * i + 1] = table[3 * i + 1]; packed[4 * i + 2] = table[3 * i + 2]; packed[4 * i + 3] = 0;
    }
}
// the five coefficients of step 2, exactly: every factor is a ratio of integers.  c: nY, nRv, nGu, nGv, nBu
inline bool lut3d_inverse(int matrix, bool full, int B, int (&c)[5])
{
    int64_t kr, kb;
    if (matrix == 1) { kr = 2126; kb = 722; }
    else if (matrix == 5 || matrix == 6) { kr = 2990; kb = 1140; }
    else if (matrix == 9) { kr = 2627; kb = 593; }
    else return false;
    const int64_t kg = 10000 - kr - kb, unit = (int64_t)1 << (B - 8), peak = ((int64_t)1 << B) - 1, one = (int64_t)65535 << 16;
    const int64_t dy = full ? peak : 219 * unit, dc = 8 * (full ? peak : 224 * unit);
    const int64_t P[5] = {one, 2 * (10000 - kr) * one, -2 * kb * (10000 - kb) * one, -2 * kr * (10000 - kr) * one, 2 * (10000 - kb) * one};      // |P| < 2^58
    const int64_t Q[5] = {dy, 10000 * dc, kg * 10000 * dc, kg * 10000 * dc, 10000 * dc};
    for (int i = 0; i < 5; i++) c[i] = (int)rgb_floor_div(2 * P[i] + Q[i], 2 * Q[i]);
    return true;
}
// every field from the source's description, the table, the geometry and the planes.  out_matrix / out_full: the session's, resolved by the caller
inline Lut3dArgs lut3d_args(const mihevc_lut3d_src &f, int n, const void *table, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int sw, int sh,
                            int pw, int ph, int out_depth, int out_matrix, bool out_full, void *const *out, const int *ostride)
{
    Lut3dArgs a;
    mihevc_rgb_format rf = {};
    rf.layout = 0; rf.r = 0; rf.g = 1; rf.b = 2; rf.sample = 0; rf.bit_depth = 16;
    a.out = ingest_rgb_args(rf, out_matrix, out_full, nullptr, nullptr, nullptr, 0, sw, sh, pw, ph, out_depth, out, ostride);
    const size_t es = f.bit_depth > 8 ? 2 : 1;
    a.src[0] = y; a.src[1] = u; a.src[2] = v;
    for (int c = 0; c < 3; c++) {
        a.pitch[c] = c ? pitch_c : pitch_y;
        a.align[c] = ingest_align(a.src[c], (size_t)a.pitch[c] * es);
    }
    a.table = table; a.n = n;
    a.vmax = (1 << f.bit_depth) - 1; a.oY = f.full_range ? 0 : 16 << (f.bit_depth - 8); a.oC8 = 8 << (f.bit_depth - 1);
    int c[5];
    lut3d_inverse(f.matrix, f.full_range != 0, f.bit_depth, c);
    a.nY = c[0]; a.nRv = c[1]; a.nGu = c[2]; a.nGv = c[3]; a.nBu = c[4];
    return a;
}

// ---- the pixel function: steps 2 and 3
// x / 65535 for x < 65535 * 65536 (every p of step 3 and every dividend of its blend)
DEV uint32_t lut_div65535(uint32_t x) { return (x + 1u + (x >> 16)) >> 16; }
DEV int lut_clip16(int64_t t)
{
    const int64_t s = (t + 32768) >> 16;
    return s < 0 ? 0 : s > 65535 ? 65535 : (int)s;
}
// step 2.  cb8, cr8: with the factor 8 of step 1.  A: what carries the two offsets and the five coefficients under these names (Lut3dArgs; sr_yuv.h's SrYuvArgs)
template <class A> DEV void lut_rgb16(const A &a, int Y, int cb8, int cr8, int (&v)[3])
{
    const int64_t y = (int64_t)a.nY * (Y - a.oY);
    const int cb = cb8 - a.oC8, cr = cr8 - a.oC8;
    v[0] = lut_clip16(y + (int64_t)a.nRv * cr);
    v[1] = lut_clip16(y + (int64_t)a.nGu * cb + (int64_t)a.nGv * cr);
    v[2] = lut_clip16(y + (int64_t)a.nBu * cb);
}
DEV void lut_vertex(const Lut3dArgs &a, int idx, uint32_t (&e)[3])
{
    const uint8_t *p = (const uint8_t *)a.table + (size_t)idx * LUT_ENTRY_BYTES;
    uint32_t w[2];
    MIHEVC_INGEST_ACCESS(p, LUT_ENTRY_BYTES);
    ingest_chunk<LUT_ENTRY_BYTES>(p, w);
    e[0] = w[0] & 0xffffu; e[1] = w[0] >> 16; e[2] = w[1] & 0xffffu;
}
// step 3: v (R', G', B' at 16 bit) through the table
DEV void lut_lookup(const Lut3dArgs &a, const int (&v)[3], int (&o)[3])
{
    const int N = a.n, step[3] = {1, N, N * N};
    uint32_t f[3];
    int idx = 0;
#pragma unroll
    for (int c = 2; c >= 0; c--) {
        const uint32_t p = (uint32_t)v[c] * (uint32_t)(N - 1);
        const uint32_t i = (uint32_t)imin((int)lut_div65535(p), N - 2);
        f[c] = p - 65535u * i;
        idx = idx * N + (int)i;
    }
    // the axis of the largest and of the smallest fraction; ties: red before green before blue for the largest, the reverse for the smallest, so the two differ
    const int s1 = f[0] >= f[1] && f[0] >= f[2] ? step[0] : f[1] >= f[2] ? step[1] : step[2];
    const int s3 = f[2] <= f[1] && f[2] <= f[0] ? step[2] : f[1] <= f[0] ? step[1] : step[0];
    const uint32_t hi = f[0] > f[1] ? f[0] : f[1], lo = f[0] < f[1] ? f[0] : f[1];
    const uint32_t f1 = hi > f[2] ? hi : f[2], f3 = lo < f[2] ? lo : f[2], f2 = f[0] + f[1] + f[2] - f1 - f3;
    const int all = step[0] + step[1] + step[2];
    uint32_t V0[3], V1[3], V2[3], V3[3];
    lut_vertex(a, idx, V0);
    lut_vertex(a, idx + s1, V1);
    lut_vertex(a, idx + all - s3, V2);
    lut_vertex(a, idx + all, V3);
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = (int)lut_div65535((65535u - f1) * V0[c] + (f1 - f2) * V1[c] + (f2 - f3) * V2[c] + f3 * V3[c] + 32767u);
}
// steps 2 to 4 (matrix) of one pixel
DEV RgbT lut_pixel(const Lut3dArgs &a, int Y, int cb8, int cr8)
{
    int v[3], o[3];
    lut_rgb16(a, Y, cb8, cr8, v);
    lut_lookup(a, v, o);
    return rgb_matrix<3>(a.out, o);
}

// ---- a 4:2:0 source in front of the pixel function
// the rows a luma row needs: its own, and of Cb and Cr the chroma row it lies in (weight 3) and the one beyond it (weight 1)
template <typename TI> struct LutRows { const TI *y, *near[2], *far[2]; };
template <typename TI> DEV int lut_element(const Lut3dArgs &a, const TI *p)
{
    int v;
    ingest_element(p, v);
    return imin(v, a.vmax);
}
// the pixel of column x of a row, element by element
template <typename TI> DEV RgbT lut_pixel_at(const Lut3dArgs &a, const LutRows<TI> &r, int x)
{
    const int cx = x >> 1, cx1 = (x & 1) ? imin(cx + 1, a.out.sw / 2 - 1) : cx;
    int c8[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int m0 = 3 * lut_element(a, r.near[c] + cx) + lut_element(a, r.far[c] + cx);
        c8[c] = m0 + ((x & 1) ? 3 * lut_element(a, r.near[c] + cx1) + lut_element(a, r.far[c] + cx1) : m0);
    }
    return lut_pixel(a, lut_element(a, r.y + x), c8[0], c8[1]);
}

// One source row of a block, as rgb_row: Y[k]: the luma of output column x0 + k; T[c][k] += the row's share of chroma output x0 / 2 + k.  y: the source luma row;
// cols: the chroma columns of the block that are stored
template <typename TI> DEV void lut_row(const Lut3dArgs &a, int y, int x0, int cols, int (&Y)[RGB_BW], int64_t (&T)[2][ING_RUN])
{
    const int sw = a.out.sw, ch = a.out.sh / 2, j = y >> 1, jf = (y & 1) ? imin(j + 1, ch - 1) : imax(j - 1, 0);
    LutRows<TI> r;
    r.y = (const TI *)a.src[0] + (ptrdiff_t)y * a.pitch[0];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        r.near[c] = (const TI *)a.src[1 + c] + (ptrdiff_t)j * a.pitch[1 + c];
        r.far[c] = (const TI *)a.src[1 + c] + (ptrdiff_t)jf * a.pitch[1 + c];
    }
    if (x0 + RGB_BW <= sw) {             // the whole block lies in the display area
        int vy[RGB_BW], m[2][ING_RUN + 1];
        ingest_load<TI, RGB_BW>(r.y + x0, a.align[0], vy);
        const int xr = imin(x0 / 2 + ING_RUN, sw / 2 - 1);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            int vn[ING_RUN], vf[ING_RUN];
            ingest_load<TI, ING_RUN>(r.near[c] + x0 / 2, a.align[1 + c], vn);
            ingest_load<TI, ING_RUN>(r.far[c] + x0 / 2, a.align[1 + c], vf);
#pragma unroll
            for (int k = 0; k < ING_RUN; k++) m[c][k] = 3 * imin(vn[k], a.vmax) + imin(vf[k], a.vmax);
            m[c][ING_RUN] = 3 * lut_element(a, r.near[c] + xr) + lut_element(a, r.far[c] + xr);
        }
        RgbT left = lut_pixel_at(a, r, imax(x0 - 1, 0));
#pragma unroll
        for (int k = 0; k < ING_RUN; k++) {
            const RgbT t0 = lut_pixel(a, imin(vy[2 * k], a.vmax), 2 * m[0][k], 2 * m[1][k]);
            const RgbT t1 = lut_pixel(a, imin(vy[2 * k + 1], a.vmax), m[0][k] + m[0][k + 1], m[1][k] + m[1][k + 1]);
            Y[2 * k] = rgb_luma(a.out, t0.y);
            Y[2 * k + 1] = rgb_luma(a.out, t1.y);
            T[0][k] += left.cb + 2 * t0.cb + t1.cb;
            T[1][k] += left.cr + 2 * t0.cr + t1.cr;
            left = t1;
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < RGB_BW; k++) Y[k] = 0;
#pragma unroll 1
    for (int k = 0; k < cols; k++) {         // the block reaches into the margin: chroma columns clamped to the display area, one element at a time
        const int i = imin(x0 / 2 + k, sw / 2 - 1);
        const RgbT l = lut_pixel_at(a, r, imax(2 * i - 1, 0)), t0 = lut_pixel_at(a, r, 2 * i), t1 = lut_pixel_at(a, r, 2 * i + 1);
        const int y1 = rgb_luma(a.out, t1.y), y0 = x0 / 2 + k == i ? rgb_luma(a.out, t0.y) : y1;      // past the display area both columns repeat the last one
#pragma unroll
        for (int q = 0; q < ING_RUN; q++)        // (no indexing of registers by k)
            if (q == k) { Y[2 * q] = y0; Y[2 * q + 1] = y1; T[0][q] += l.cb + 2 * t0.cb + t1.cb; T[1][q] += l.cr + 2 * t0.cr + t1.cr; }
    }
}

// the lane's block of tile `tile`: luma rows 2j and 2j + 1, chroma row j (the cut and the margin rule of rgb_block)
template <typename TI, typename TO> DEV void lut_block(const Lut3dArgs &a, int tile, int tid)
{
    const IngestRgbArgs &g = a.out;
    const int ntx = (g.pw + RGB_TW - 1) / RGB_TW, ty = tile / ntx, tx = tile - ty * ntx;
    const int x0 = (tx * RGB_LX + (tid & (RGB_LX - 1))) * RGB_BW, j = ty * RGB_LY + tid / RGB_LX;
    if (x0 >= g.pw || 2 * j >= g.ph) return;
    const bool inside = j < g.sh / 2, wide = x0 + RGB_BW <= g.pw;      // below the display area the block reads the last two rows; wide: both runs of a luma row
    const int js = inside ? j : g.sh / 2 - 1;
    int64_t T[2][ING_RUN];
#pragma unroll
    for (int k = 0; k < ING_RUN; k++) T[0][k] = T[1][k] = 0;
    auto store_luma = [&](int y, const int (&Y)[RGB_BW]) {
        TO *p = (TO *)g.dst[0] + (ptrdiff_t)y * g.dstride[0] + x0;
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
        lut_row<TI>(a, 2 * js + r, x0, wide ? ING_RUN : ING_RUN / 2, Y, T);
        if (r || inside) store_luma(2 * j + r, Y);
        if (r && !inside) store_luma(2 * j, Y);      // both luma rows repeat the last source row
    }
#pragma unroll
    for (int c = 0; c < 2; c++) {
        int o[ING_RUN];
#pragma unroll
        for (int k = 0; k < ING_RUN; k++) o[k] = rgb_chroma(g, T[c][k]);
        ingest_store((TO *)g.dst[1 + c] + (ptrdiff_t)j * g.dstride[1 + c] + x0 / 2, o, wide);
    }
}

// workgroup `wg` of the launch
template <typename TI, typename TO, class Ex> DEV void lut3d_tile_program(Ex &ex, const Lut3dArgs &a, int wg)
{
    if (wg >= ingest_rgb_workgroups(a.out.pw, a.out.ph)) return;
    ex.phase([&](int tid) { lut_block<TI, TO>(a, wg, tid); });
}

}  // namespace mihevc
