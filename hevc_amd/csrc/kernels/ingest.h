// hevc_amd/csrc/kernels/ingest.h — source conversion (mihevc_send_frame_fmt, mihevc_k_convert_source): a 4:2:0 / 4:2:2 / 4:4:4, planar or semi-planar, 8 .. 16 bit
// source picture -> the session's own planar 4:2:0 planes at 8 or 10 bit, margin included.  Integers only, so that the device, the stepped kernel (tests/emu)
// and the numpy model (tests/ingest_ref.py) agree bit for bit.  R'G'B' sources take the same road with a colour matrix in front: ingest_rgb.h, which builds on
// the loads, stores and alignment classes of this file.  The definition (normative; DESIGN.md repeats it):
//   picture  W x H (display size, both even); chroma planes W/2 x H/2 (420), W/2 x H (422), W x H (444).  B = significant bits of a source sample (8 .. 16),
//            D = the session's bit depth (8 or 10)
//   sample   the raw element r is a uint8 when B == 8, else a little-endian uint16.  msb_aligned (P010, P210 ...): v = r >> (16 - B); else v = min(r, 2^B - 1)
//   chroma   sum S with weight 2^k of output chroma sample (i, j):
//              420  S = c[j][i], k = 0
//              422  S = c[2j][i] + c[2j+1][i], k = 1
//              444  S = sum over r in {2j, 2j+1} of (c[r][max(2i-1, 0)] + 2 c[r][2i] + c[r][2i+1]), k = 3
//            (the siting of chroma_sample_loc_type 0: horizontally co-sited with the even luma column, vertically midway).  Luma: S = v, k = 0
//   depth    n = k + max(0, B - D), m = max(0, D - B); out = min(((S << m) + ((1 << n) >> 1)) >> n, 2^D - 1): rounded half up, once, after the filter.
//            Everything fits 32 bits (8 * 65535 << 2)
//   margin   the output planes have the CODED size (display size rounded up to 8); output sample (x, y) outside the display area equals the output sample at
//            (min(x, sw - 1), min(y, sh - 1)): what k_extend_margin leaves
//   semi-planar  `u` is one plane with Cb in its even and Cr in its odd elements, pitch_c in elements of that plane; `v` is not read
// One launch per picture (k_ingest), no LDS: a workgroup takes one tile of ING_TW x ING_TH output samples, the tiles of Y first, then Cb, then Cr (a semi-planar
// source: the Cb tiles write Cr too, so the interleaved plane is read once, and there are no Cr tiles).  A lane produces ING_RUN adjacent output samples of one
// row and stores them with one 8-byte (uint8) or 16-byte (uint16) store (the last run of a chroma row may be half a run: coded chroma widths are multiples of
// 4); lanes side by side take runs side by side.  A run inside the display area reads its source rows in chunks of 16, 8 or 4 bytes, the widest the plane's
// base address and pitch allow (IngestArgs::align, the same for every lane: a uniform branch), or element by element; a run that reaches into the margin, and
// the left tap of the 4:4:4 filter, read single elements at clamped coordinates.  No access the source states is wider than its alignment (the stepped harness counts them) and none lies outside
// the rows of the source; what the compiler makes of the narrow paths on the device is kept apart by ingest_keep_apart: the device tests run every alignment
// class and check what comes out, not the width of the accesses.  ingest_load, ingest_element and ingest_store serve k_ingest_rgb too: one copy of the
// chunk paths, behind one access hook.
#pragma once
#include "common.h"

namespace mihevc {

constexpr int ING_RUN = 8;                         // output samples per lane
constexpr int ING_LX = 16, ING_LY = NT / ING_LX;   // lanes of a workgroup: 16 runs side by side x 16 rows
constexpr int ING_TW = ING_LX * ING_RUN, ING_TH = ING_LY;

struct IngestArgs {
    const void *src[3];      // Y, Cb (semi-planar: the interleaved plane), Cr (semi-planar: unused)
    void *dst[3];            // coded-size planes; 16-byte aligned, strides too
    int pitch[3];            // source, in elements (of the interleaved plane)
    int dstride[3];          // in samples
    int align[3];            // per source plane: 16, 8, 4 or 1 (ingest_align)
    int sw, sh, pw, ph;      // display and coded size of luma
    int chroma, semi;        // 420 / 422 / 444; 1: semi-planar
    int shift, vmax;         // v = min(r >> shift, vmax)
    int m, n_y, n_c, peak;   // out = min(((S << m) + ((1 << n) >> 1)) >> n, peak)
};

HDI bool src_format_ok(const mihevc_src_format *f)
{
    if (!f || (f->chroma != 420 && f->chroma != 422 && f->chroma != 444) || (f->semi_planar != 0 && f->semi_planar != 1)) return false;
    if (f->bit_depth < 8 || f->bit_depth > 16 || (f->msb_aligned != 0 && f->msb_aligned != 1) || (f->msb_aligned && f->bit_depth == 8)) return false;
    return !(f->reserved[0] | f->reserved[1] | f->reserved[2] | f->reserved[3]);
}
// size of a source chroma plane in ELEMENTS per row (both components of an interleaved plane) and in rows
HDI int src_chroma_row(const mihevc_src_format &f, int w) { return (f.chroma == 444 ? w : w / 2) * (f.semi_planar ? 2 : 1); }
HDI int src_chroma_rows(const mihevc_src_format &f, int h) { return f.chroma == 420 ? h / 2 : h; }
// the widest chunk every run of a plane may be read with: a power of two that divides the base address and the pitch in bytes
HDI int ingest_align(const void *p, size_t pitch_bytes)
{
    const size_t v = (size_t)(uintptr_t)p | pitch_bytes;
    return !(v & 15) ? 16 : !(v & 7) ? 8 : !(v & 3) ? 4 : 1;
}
HDI int ingest_tiles(int w, int h) { return ((w + ING_TW - 1) / ING_TW) * ((h + ING_TH - 1) / ING_TH); }
HDI int ingest_workgroups(int pw, int ph, int semi) { return ingest_tiles(pw, ph) + (semi ? 1 : 2) * ingest_tiles(pw / 2, ph / 2); }
// workgroup r -> component (0 Y, 1 Cb, 2 Cr), r becomes the tile inside it; -1 past the last
HDI int ingest_locate(int pw, int ph, int semi, int &r)
{
    const int ny = ingest_tiles(pw, ph), nc = ingest_tiles(pw / 2, ph / 2);
    if (r < ny) return 0;
    r -= ny;
    if (r < nc) return 1;
    r -= nc;
    return !semi && r < nc ? 2 : -1;
}
// every field from the format, the geometry and the planes.  y, u, v / pitch_*: the source; out / ostride: the coded-size planes
inline IngestArgs ingest_args(const mihevc_src_format &f, const void *y, const void *u, const void *v, int pitch_y, int pitch_c, int sw, int sh, int pw, int ph,
                              int out_depth, void *const *out, const int *ostride)
{
    IngestArgs a;
    const size_t es = f.bit_depth > 8 ? 2 : 1;
    a.src[0] = y; a.src[1] = u; a.src[2] = f.semi_planar ? nullptr : v;
    for (int c = 0; c < 3; c++) {
        a.dst[c] = out[c]; a.dstride[c] = ostride[c]; a.pitch[c] = c ? pitch_c : pitch_y;
        a.align[c] = a.src[c] ? ingest_align(a.src[c], (size_t)a.pitch[c] * es) : 1;
    }
    a.sw = sw; a.sh = sh; a.pw = pw; a.ph = ph; a.chroma = f.chroma; a.semi = f.semi_planar;
    a.shift = f.msb_aligned ? 16 - f.bit_depth : 0; a.vmax = (1 << f.bit_depth) - 1;
    const int down = f.bit_depth > out_depth ? f.bit_depth - out_depth : 0;
    a.m = out_depth > f.bit_depth ? out_depth - f.bit_depth : 0;
    a.n_y = down; a.n_c = down + (f.chroma == 444 ? 3 : f.chroma == 422 ? 1 : 0); a.peak = (1 << out_depth) - 1;
    return a;
}

// every chunk load, every load through ingest_element and every store passes here with its address and its width in bytes: nothing in the product; the stepped
// harnesses (tests/emu/ingest_planes.h) define the hook before they include this file and count the accesses whose address is not a multiple of their width
#ifndef MIHEVC_INGEST_ACCESS
#define MIHEVC_INGEST_ACCESS(p, bytes) ((void)0)
#endif

// Between the accesses of a narrow path.  gfx950 serves misaligned global accesses, and the compiler knows: left alone it fuses the adjacent element or
// 4- / 8-byte loads of a narrow path back into dwordx4 loads at whatever address.  The narrow paths exist so that no access is wider than its alignment
DEV void ingest_keep_apart()
{
#if MIHEVC_GPU
    asm volatile("" ::: "memory");
#endif
}
// one aligned access of CB bytes, as a vector of dwords: two memcpy of different lengths in two branches end as dword accesses shared between them
typedef uint32_t ingest_u32x2 __attribute__((vector_size(8), may_alias));
typedef uint32_t ingest_u32x4 __attribute__((vector_size(16), may_alias));
template <int CB> DEV void ingest_chunk(const void *p, uint32_t (&w)[CB / 4])
{
    if constexpr (CB == 16) {
        const ingest_u32x4 v = *(const ingest_u32x4 *)__builtin_assume_aligned(p, 16);
        w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
    } else if constexpr (CB == 8) {
        const ingest_u32x2 v = *(const ingest_u32x2 *)__builtin_assume_aligned(p, 8);
        w[0] = v[0]; w[1] = v[1];
    } else w[0] = load_u32_aligned(p);
}
// one element, kept apart from its neighbours: the narrowest path of ingest_load, and the single pixels of k_ingest_rgb
template <typename TI> DEV void ingest_element(const TI *p, int &v)
{
    MIHEVC_INGEST_ACCESS(p, sizeof(TI));
    v = (int)*p;
    ingest_keep_apart();
}
// N elements from p in chunks of CB bytes (p is CB-aligned)
template <typename TI, int N, int CB> DEV void ingest_load_chunks(const TI *p, int (&v)[N])
{
    constexpr int per = CB / (int)sizeof(TI);
#pragma unroll
    for (int c = 0; c < N / per; c++) {
        uint32_t w[CB / 4];
        MIHEVC_INGEST_ACCESS(p + c * per, CB);
        ingest_chunk<CB>(p + c * per, w);
        if constexpr (CB < 16) ingest_keep_apart();
#pragma unroll
        for (int k = 0; k < per; k++) {
            if constexpr (sizeof(TI) == 1) v[c * per + k] = (int)((w[k >> 2] >> (8 * (k & 3))) & 255u);
            else if constexpr (sizeof(TI) == 2) v[c * per + k] = (int)((w[k >> 1] >> (16 * (k & 1))) & 0xffffu);
            else v[c * per + k] = (int)w[k];
        }
    }
}
// N elements of one row; al: the plane's IngestArgs::align; the offset of p in its row is a multiple of N elements
template <typename TI, int N> DEV void ingest_load(const TI *p, int al, int (&v)[N])
{
    if constexpr (N * sizeof(TI) >= 16) {
        if (al >= 16) { ingest_load_chunks<TI, N, 16>(p, v); return; }
    }
    if (al >= 8) { ingest_load_chunks<TI, N, 8>(p, v); return; }
    if (al >= 4) { ingest_load_chunks<TI, N, 4>(p, v); return; }
#pragma unroll
    for (int k = 0; k < N; k++) ingest_element(p + k, v[k]);
}

// ING_RUN samples (`full`), or the first half of them, to p: one vector store either way
DEV void ingest_store(uint8_t *p, const int (&o)[ING_RUN], bool full)
{
    const uint32_t w0 = (uint32_t)o[0] | (uint32_t)o[1] << 8 | (uint32_t)o[2] << 16 | (uint32_t)o[3] << 24;
    const uint32_t w1 = (uint32_t)o[4] | (uint32_t)o[5] << 8 | (uint32_t)o[6] << 16 | (uint32_t)o[7] << 24;
    MIHEVC_INGEST_ACCESS(p, full ? 8 : 4);
    if (full) *(ingest_u32x2 *)__builtin_assume_aligned(p, 8) = ingest_u32x2{w0, w1};
    else store_u32_aligned(p, w0);
}
DEV void ingest_store(uint16_t *p, const int (&o)[ING_RUN], bool full)
{
    const uint32_t w0 = (uint32_t)o[0] | (uint32_t)o[1] << 16, w1 = (uint32_t)o[2] | (uint32_t)o[3] << 16;
    const uint32_t w2 = (uint32_t)o[4] | (uint32_t)o[5] << 16, w3 = (uint32_t)o[6] | (uint32_t)o[7] << 16;
    MIHEVC_INGEST_ACCESS(p, full ? 16 : 8);
    if (full) *(ingest_u32x4 *)__builtin_assume_aligned(p, 16) = ingest_u32x4{w0, w1, w2, w3};
    else *(ingest_u32x2 *)__builtin_assume_aligned(p, 8) = ingest_u32x2{w0, w1};
}

// One source row's share of the sums of a run: S[c][k] += the row's term of output sample x0 + k of component c.  NC: components side by side in the row
// (2: an interleaved plane); H: the 1-2-1 filter of 4:4:4 with 2:1 decimation.  row: the first element of the source row; swo: display width of the OUTPUT plane
template <typename TI, int NC, bool H> DEV void ingest_row(const TI *row, int x0, int swo, int al, int shift, int vmax, int (&S)[NC][ING_RUN])
{
    auto sample = [&](ptrdiff_t i) { return imin((int)row[i] >> shift, vmax); };
    if (x0 + ING_RUN <= swo) {           // the whole run lies in the display area
        constexpr int N = ING_RUN * NC * (H ? 2 : 1);
        int v[N];
        ingest_load<TI, N>(row + (ptrdiff_t)x0 * (N / ING_RUN), al, v);
#pragma unroll
        for (int i = 0; i < N; i++) v[i] = imin(v[i] >> shift, vmax);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if constexpr (H) {
                const int left = sample((ptrdiff_t)imax(2 * x0 - 1, 0) * NC + c);
#pragma unroll
                for (int k = 0; k < ING_RUN; k++) S[c][k] += (k ? v[(2 * k - 1) * NC + c] : left) + 2 * v[2 * k * NC + c] + v[(2 * k + 1) * NC + c];
            } else {
#pragma unroll
                for (int k = 0; k < ING_RUN; k++) S[c][k] += v[k * NC + c];
            }
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < ING_RUN; k++) {      // the run reaches into the margin: columns clamped to the display area, one element at a time
        const int i = imin(x0 + k, swo - 1);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if constexpr (H) S[c][k] += sample((ptrdiff_t)imax(2 * i - 1, 0) * NC + c) + 2 * sample((ptrdiff_t)2 * i * NC + c) + sample((ptrdiff_t)(2 * i + 1) * NC + c);
            else S[c][k] += sample((ptrdiff_t)i * NC + c);
        }
    }
}

// the lane's run of component c (NC == 2: of Cb and Cr) in tile `tile`
template <typename TI, typename TO, int NC, bool H> DEV void ingest_run(const IngestArgs &a, int c, int tile, int tid)
{
    const int swo = c ? a.sw / 2 : a.sw, sho = c ? a.sh / 2 : a.sh, pwo = c ? a.pw / 2 : a.pw, pho = c ? a.ph / 2 : a.ph;
    const int ntx = (pwo + ING_TW - 1) / ING_TW, ty = tile / ntx, tx = tile - ty * ntx;
    const int x0 = (tx * ING_LX + (tid & (ING_LX - 1))) * ING_RUN, y = ty * ING_TH + tid / ING_LX;
    if (x0 >= pwo || y >= pho) return;
    const int rows = c && a.chroma != 420 ? 2 : 1, y0 = imin(y, sho - 1) * rows, n = c ? a.n_c : a.n_y;
    int S[NC][ING_RUN];
#pragma unroll
    for (int q = 0; q < NC; q++)
#pragma unroll
        for (int k = 0; k < ING_RUN; k++) S[q][k] = 0;
    const TI *src = (const TI *)a.src[c];
    for (int r = 0; r < rows; r++) ingest_row<TI, NC, H>(src + (ptrdiff_t)(y0 + r) * a.pitch[c], x0, swo, a.align[c], a.shift, a.vmax, S);
    const bool full = x0 + ING_RUN <= pwo;
#pragma unroll
    for (int q = 0; q < NC; q++) {
        int o[ING_RUN];
#pragma unroll
        for (int k = 0; k < ING_RUN; k++) o[k] = imin(((S[q][k] << a.m) + ((1 << n) >> 1)) >> n, a.peak);
        ingest_store((TO *)a.dst[c + q] + (ptrdiff_t)y * a.dstride[c + q] + x0, o, full);
    }
}

// workgroup `wg` of the launch
template <typename TI, typename TO, class Ex> DEV void ingest_tile_program(Ex &ex, const IngestArgs &a, int wg)
{
    int tile = wg;
    const int c = ingest_locate(a.pw, a.ph, a.semi, tile);
    if (c < 0) return;
    ex.phase([&](int tid) {
        if (c == 0) ingest_run<TI, TO, 1, false>(a, 0, tile, tid);
        else if (a.chroma == 444) {
            if (a.semi) ingest_run<TI, TO, 2, true>(a, 1, tile, tid);
            else ingest_run<TI, TO, 1, true>(a, c, tile, tid);
        } else {
            if (a.semi) ingest_run<TI, TO, 2, false>(a, 1, tile, tid);
            else ingest_run<TI, TO, 1, false>(a, c, tile, tid);
        }
    });
}

}  // namespace mihevc
