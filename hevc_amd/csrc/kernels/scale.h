// hevc_amd/csrc/kernels/scale.h — downscaling source (mihevc_send_frame_scaled, mihevc_k_scale_source): a planar 4:2:0 picture of sw x sh samples at 8 .. 16
// bit -> the session's own planar 4:2:0 planes of dw x dh (dw <= sw <= 4 dw, dh <= sh <= 4 dh) at 8 or 10 bit, margin included.  A separable polyphase filter,
// integers only, so that the device, the stepped kernel (tests/emu/scale.cpp) and the numpy model (tests/scale_ref.py) agree bit for bit.  The definition
// (normative: DESIGN.md §6e; the coefficient tables: csrc/scale_taps.h):
//   sample      the raw element r is a uint8 when B == 8, else a little-endian uint16; v = min(r, 2^B - 1)
//   tables      per axis of a plane, output sample i has a first source index f_i and 16 coefficients c_0 .. c_15 that sum to 4096 (zero padded)
//   horizontal  first: m = (sum_j c_j v[clamp(f_i + j, 0, S - 1)] + 2^(11-G)) >> (12 - G), G = min(4, 16 - B) guard bits; m is signed and NOT clamped
//   vertical    on m: T = sum_j c_j m[clamp(f_i + j, 0, S - 1)], n = 12 + G + max(0, B - D), u = max(0, D - B),
//               out = clamp((T 2^u + 2^(n-1)) >> n, 0, 2^D - 1)          (>>: arithmetic, rounds down)
//   margin      as ingest.h: output sample (x, y) outside the display area equals the output sample at (min(x, dw - 1), min(y, dh - 1))
//   32 bits     sum |c_j| <= 6144 per row (scale_taps_build refuses otherwise): |sum c v| <= 6144 * 65535, |T 2^u| <= 6144 * 1.5 * 2^16
// One launch per picture (k_scale): a workgroup takes one tile of SC_TW x SC_TH output samples of one plane, the tiles of Y first, then Cb, then Cr.  Phase 1
// filters horizontally every source row the tile's output rows have a tap in (at most SC_ROWS = 4 SC_TH + 16 of them, rows clamped into the plane) into LDS,
// 32 bits a sample (m overshoots 16 bits at B == 16); HBM never sees it.  A lane keeps one output column's coefficients in registers and walks down the rows; the
// lanes of a wave take adjacent columns, so the 64 elements one tap reads lie r = S / Dn apart in one to four cache lines (512 bytes at 4:1 on 16-bit samples).  The raw source window is NOT staged in LDS:
// the taps of adjacent outputs overlap and the L1 serves the repeats, while a staged window would have to be indexed per lane at a run-time offset (a gather
// from LDS at element width, its banks conflicting at every ratio that is not 1:1) to save loads that already hit.  Every global read is therefore one element
// through ingest_element at a clamped column of a clamped row: never wider than the element, never outside the source rows, whatever the planes' alignment.
// Phase 2 filters vertically out of LDS: a lane produces ING_RUN adjacent output samples of one row from two 16-byte LDS reads per tap and stores them with one
// ingest_store.  Rows of the image are 512 bytes, so the lanes of one ds_read_b128 group (16 lanes, eight of one output row and eight of the next) would meet
// two by two on the same 16-byte slot; lanes of odd rows read the upper half of their run first, which puts the two rows of a group on alternate slots.
#pragma once
#include "ingest.h"

namespace mihevc {

constexpr int SC_LX = 16, SC_LY = NT / SC_LX;                 // lanes of phase 2: 16 runs side by side x 16 rows
constexpr int SC_TW = SC_LX * ING_RUN, SC_TH = SC_LY;         // the tile: 128 x 16 output samples
constexpr int SC_ROWS = 4 * SC_TH + 16;                       // horizontally filtered rows a tile can need (4:1)
constexpr int SC_TAPS = 16;

struct ScaleShared {
    int32_t m[SC_ROWS][SC_TW];      // 40,960 bytes
};

struct ScaleArgs {
    const void *src[3];             // Y, Cb, Cr of the source
    void *dst[3];                   // coded-size planes; 16-byte aligned, strides too
    int pitch[3];                   // source, in elements
    int dstride[3];                 // in samples
    int sw, sh;                     // source size (luma)
    int dw, dh, pw, ph;             // display and coded size of the output (luma)
    const int32_t *first[4];        // tables: 0 luma horizontal, 1 luma vertical, 2 chroma horizontal, 3 chroma vertical; per output sample of the axis
    const int16_t *coef[4];         // SC_TAPS per output sample, rows 16-byte aligned
    int taps[4];                    // the longest row of each table
    int vmax;                       // v = min(r, vmax)
    int hround, hshift;             // m = (sum + hround) >> hshift
    int n, u, peak;                 // out = clamp((T << u) + (1 << (n - 1)) >> n, 0, peak)
};

HDI bool scale_geometry_ok(int sw, int sh, int dw, int dh)
{
    return sw >= 16 && sh >= 16 && dw >= 16 && dh >= 16 && !((sw | sh | dw | dh) & 1) && dw <= sw && sw <= 4 * dw && dh <= sh && sh <= 4 * dh;
}
HDI bool scale_src_ok(const mihevc_scale_src *f)
{
    if (!f || f->bit_depth < 8 || f->bit_depth > 16) return false;
    return !(f->reserved[0] | f->reserved[1] | f->reserved[2] | f->reserved[3] | f->reserved[4]);
}
HDI int scale_tiles(int w, int h) { return ((w + SC_TW - 1) / SC_TW) * ((h + SC_TH - 1) / SC_TH); }
HDI int scale_workgroups(int pw, int ph) { return scale_tiles(pw, ph) + 2 * scale_tiles(pw / 2, ph / 2); }
// workgroup r -> component (0 Y, 1 Cb, 2 Cr), r becomes the tile inside it; -1 past the last
HDI int scale_locate(int pw, int ph, int &r)
{
    const int ny = scale_tiles(pw, ph), nc = scale_tiles(pw / 2, ph / 2);
    if (r < ny) return 0;
    r -= ny;
    if (r < nc) return 1;
    r -= nc;
    return r < nc ? 2 : -1;
}
// every field from the geometry, the planes and the tables (first / coef / taps as ScaleArgs: where the kernel will read them).  B: bits of a source sample
inline ScaleArgs scale_args(int B, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int sw, int sh, int dw, int dh, int pw, int ph, int out_depth,
                            void *const *out, const int *ostride, const int32_t *const *first, const int16_t *const *coef, const int *taps)
{
    ScaleArgs a;
    a.src[0] = y; a.src[1] = u; a.src[2] = v;
    for (int c = 0; c < 3; c++) { a.dst[c] = out[c]; a.dstride[c] = ostride[c]; a.pitch[c] = c ? pitch_c : pitch_y; }
    for (int k = 0; k < 4; k++) { a.first[k] = first[k]; a.coef[k] = coef[k]; a.taps[k] = taps[k]; }
    a.sw = sw; a.sh = sh; a.dw = dw; a.dh = dh; a.pw = pw; a.ph = ph;
    const int G = 16 - B < 4 ? 16 - B : 4;
    a.vmax = (1 << B) - 1;
    a.hshift = 12 - G; a.hround = 1 << (11 - G);
    a.n = 12 + G + (B > out_depth ? B - out_depth : 0); a.u = out_depth > B ? out_depth - B : 0; a.peak = (1 << out_depth) - 1;
    return a;
}

// coefficient j of a row held as eight dwords
DEV int scale_coef(const uint32_t (&cw)[SC_TAPS / 2], int j) { return (int)(int16_t)(cw[j >> 1] >> (16 * (j & 1))); }
DEV void scale_coef_row(const int16_t *row, uint32_t (&cw)[SC_TAPS / 2])
{
    const ingest_u32x4 lo = *(const ingest_u32x4 *)__builtin_assume_aligned(row, 16), hi = *(const ingest_u32x4 *)__builtin_assume_aligned(row + 8, 16);
#pragma unroll
    for (int k = 0; k < 4; k++) { cw[k] = lo[k]; cw[4 + k] = hi[k]; }
}
typedef int32_t scale_i32x4 __attribute__((vector_size(16), may_alias));

// workgroup `wg` of the launch
template <typename TI, typename TO, class Ex> DEV void scale_tile_program(Ex &ex, ScaleShared &s, const ScaleArgs &a, int wg)
{
    int tile = wg;
    const int c = scale_locate(a.pw, a.ph, tile);
    if (c < 0) return;
    // Every field is read here, once: the phases below read none.  (Reads of `a` inside the unrolled tap loops, one per tap behind ingest_element's compiler
    // barrier, are more uses than the compiler follows when it folds the kernel's private copy of the argument block away: it then stays, in scratch)
    const int th = c ? 2 : 0, tv = th + 1;                                                              // the plane's tables
    const int32_t *const first_h = a.first[th], *const first_v = a.first[tv];
    const int16_t *const coef_h = a.coef[th], *const coef_v = a.coef[tv];
    const int taps_h = a.taps[th], taps_v = a.taps[tv];
    const TI *const src = (const TI *)a.src[c];
    TO *const dst = (TO *)a.dst[c];
    const int pitch_c = a.pitch[c], dstride_c = a.dstride[c];
    const int vmax = a.vmax, hround = a.hround, hshift = a.hshift, peak = a.peak, up = 1 << a.u, n = a.n;
    const int ssw = c ? a.sw / 2 : a.sw, ssh = c ? a.sh / 2 : a.sh;                                     // source plane
    const int dwo = c ? a.dw / 2 : a.dw, dho = c ? a.dh / 2 : a.dh, pwo = c ? a.pw / 2 : a.pw, pho = c ? a.ph / 2 : a.ph;
    const int ntx = (pwo + SC_TW - 1) / SC_TW, ty = tile / ntx, tx = tile - ty * ntx;
    const int y_first = imin(ty * SC_TH, dho - 1), y_last = imin(ty * SC_TH + SC_TH, dho) - 1;
    const int k0 = first_v[y_first];                                                                // source row of LDS row 0 (before clamping)
    const int nrows = imin(first_v[imax(y_last, y_first)] + taps_v - k0, SC_ROWS);
    ex.phase([&](int tid) {          // horizontal: column tid % SC_TW of rows tid / SC_TW, + 2, ...
        const int col = tid & (SC_TW - 1), i = imin(tx * SC_TW + col, dwo - 1), f = first_h[i], nt = taps_h;
        uint32_t cw[SC_TAPS / 2];
        scale_coef_row(coef_h + (ptrdiff_t)i * SC_TAPS, cw);
        for (int l = tid / SC_TW; l < nrows; l += NT / SC_TW) {
            const TI *row = src + (ptrdiff_t)clip3(0, ssh - 1, k0 + l) * pitch_c;
            int v[SC_TAPS], sum = hround;
#pragma unroll
            for (int j = 0; j < SC_TAPS; j++)      // every load of the row first: with the arithmetic beside its load a lane waits for memory once per tap
                if (j < nt) ingest_element(row + clip3(0, ssw - 1, f + j), v[j]);      // (uniform; a break would keep the loop rolled and the registers indexed at run time)
#pragma unroll
            for (int j = 0; j < SC_TAPS; j++)
                if (j < nt) sum += scale_coef(cw, j) * imin(v[j], vmax);
            s.m[l][col] = sum >> hshift;
        }
    });
    ex.phase([&](int tid) {          // vertical: the lane's run of ING_RUN samples
        const int lx = tid & (SC_LX - 1), ly = tid / SC_LX, cx = lx * ING_RUN, x0 = tx * SC_TW + cx, y = ty * SC_TH + ly;
        if (x0 >= pwo || y >= pho) return;
        const int i = imin(y, dho - 1), l0 = first_v[i] - k0, nt = taps_v, h = (ly & 1) * 4;
        uint32_t cw[SC_TAPS / 2];
        scale_coef_row(coef_v + (ptrdiff_t)i * SC_TAPS, cw);
        int T[ING_RUN];              // T[0 .. 3]: columns h .. h + 3 of the run, T[4 .. 7]: the other half
#pragma unroll
        for (int k = 0; k < ING_RUN; k++) T[k] = 0;
#pragma unroll
        for (int j = 0; j < SC_TAPS; j++) {
            if (j < nt) {
                // nt is the table's LONGEST row: a shorter row reads on past its own taps and relies on its zero padding (exact in integers; a float or
                // packed variant must not inherit that).  What it reads was written: l0 + j < first_v[y_last] + nt - k0 = nrows.  The imin only guards the image
                const int32_t *r = &s.m[imin(l0 + j, SC_ROWS - 1)][cx];
                const scale_i32x4 p = *(const scale_i32x4 *)__builtin_assume_aligned(r + h, 16), q = *(const scale_i32x4 *)__builtin_assume_aligned(r + 4 - h, 16);
                const int cj = scale_coef(cw, j);
#pragma unroll
                for (int k = 0; k < 4; k++) { T[k] += cj * p[k]; T[4 + k] += cj * q[k]; }
            }
        }
        int o[ING_RUN];
#pragma unroll
        for (int k = 0; k < ING_RUN; k++) {
            const int t = h ? T[k ^ 4] : T[k];
            o[k] = clip3(0, peak, (t * up + (1 << (n - 1))) >> n);
        }
        ingest_store(dst + (ptrdiff_t)y * dstride_c + x0, o, x0 + ING_RUN <= pwo);
    });
}

}  // namespace mihevc
