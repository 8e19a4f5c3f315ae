// hevc_amd/csrc/kernels/deint.h — deinterlacing source (mihevc_send_frame_deint, mihevc_k_deinterlace): three woven interlaced frames P (previous), C (current),
// N (next), planar 4:2:0 at the session's own depth B (8 or 10) -> one progressive picture in the session's planes, margin included.  A motion-adaptive,
// edge-directed filter in the manner of yadif, defined in integers so that the device, the stepped kernel (tests/emu/deint.cpp) and the numpy model
// (tests/deint_ref.py) agree bit for bit; it is not claimed to match any other implementation digit for digit.  The definition (normative: DESIGN.md §6f):
//   sample    the raw element r is a uint8 when B == 8, else a little-endian uint16; v = min(r, 2^B - 1)
//   planes    Y, Cb and Cr are filtered each on its own with the same keep and second (in interlaced 4:2:0 the chroma rows alternate fields as the luma rows do)
//   keep      parity of the rows that are kept (0: even rows, the top field); second: 1 when the kept field is the later of its frame's two fields in time
//   geometry  the plane is W x H, H >= 4 and even (luma: W even, H a multiple of 4, both >= 16); column indices are clamped to [0, W - 1]; a row index r < 0 is
//             replaced by r + 2 and r >= H by r - 2, which preserves its parity
//   kept      out[y][x] = C[y][x] for (y & 1) == keep
//   missing   A = second ? C : P, Z = second ? N : C: the two nearest fields of the missing parity.  Signed ints, >> arithmetic:
//               c = C[y-1][x]   e = C[y+1][x]   d = (A[y][x] + Z[y][x]) >> 1
//               t0 = |A[y][x] - Z[y][x]|
//               t1 = (|P[y-1][x] - c| + |P[y+1][x] - e|) >> 1
//               t2 = (|N[y-1][x] - c| + |N[y+1][x] - e|) >> 1
//               diff = max(t0 >> 1, t1, t2)
//               score(j) = sum over k in {-1, 0, 1} of |C[y-1][x+k+j] - C[y+1][x+k-j]|        pred(j) = (C[y-1][x+j] + C[y+1][x-j]) >> 1
//               best = score(0) - 1; sp = pred(0)
//               for s in (-1, +1), in this order: if score(s) < best { best = score(s); sp = pred(s); if score(2s) < best { best = score(2s); sp = pred(2s) } }
//               b = (A[y-2][x] + Z[y-2][x]) >> 1        f = (A[y+2][x] + Z[y+2][x]) >> 1
//               mx = max(d - e, d - c, min(b - c, f - e))        mn = min(d - e, d - c, max(b - c, f - e))
//               diff = max(diff, mn, -mx)
//               out[y][x] = sp > d + diff ? d + diff : sp < d - diff ? d - diff : sp
//             (A and Z enter only as A + Z and |A - Z|: the kernel reads C and X = second ? N : P.)  The result lies in [0, 2^B - 1]: no final clamp
//   margin    as ingest.h: output sample (x, y) outside the display area equals the output sample at (min(x, W - 1), min(y, H - 1))
// One launch per output picture (k_deint): a workgroup takes one tile of DI_TW x DI_TH output samples of one plane, the tiles of Y first, then Cb, then Cr.
// Phase 1 stages the tile's rows of C, two more above and below and one run either side (three columns are needed; a whole run keeps the image's runs on the
// plane's runs), in LDS as 16-bit samples, clamped in value, column and row: runs inside the plane come through ingest_load at the planes' alignment class,
// the others element by element at clamped columns.  Phase 2: a lane takes one run of ING_RUN columns of one PAIR of rows, so every lane has one kept row (a
// copy out of LDS) and one missing row (the filter): copy lanes and filter lanes never sit in different waves.  For the missing row the lane reads C[y-1] and
// C[y+1] at columns x0 - 8 .. x0 + 15 with three 16-byte LDS reads each (the five score / pred offsets reach x - 3 .. x + 3; nothing is loaded again per
// offset), C[y-2], C[y], C[y+2] with one each, and seven runs from memory: P[y-1], P[y+1], N[y-1], N[y+1], X[y-2], X[y], X[y+2].  Rows of P, X and N are read
// by the lanes of two (three) neighbouring row pairs; the repeats are L1 / L2 hits inside the workgroup's tile.  A run that reaches past W reads its elements
// one by one at clamped columns; the samples past W then copy the last one inside.  No access is wider than the planes' alignment and none lies outside the
// caller's rows: a plane may end with its last sample.  Every run starts inside the display area (coded - display < one run, and runs start on multiples of it).
#pragma once
#include "ingest.h"

namespace mihevc {

constexpr int DI_LX = 16, DI_LY = NT / DI_LX;                     // lanes of phase 2: 16 runs side by side x 16 row pairs
constexpr int DI_TW = DI_LX * ING_RUN, DI_TH = 2 * DI_LY;         // the tile: 128 x 32 output samples
constexpr int DI_LW = DI_TW + 2 * ING_RUN, DI_LH = DI_TH + 4;     // the LDS image of C: 144 x 36
constexpr int DI_RUNS = DI_LW / ING_RUN;

struct DeintShared {
    uint16_t c[DI_LH][DI_LW];       // 10,368 bytes; row l is row ty * DI_TH - 2 + l of the plane, column i is column tx * DI_TW - ING_RUN + i
};

struct DeintArgs {
    const void *prev[3], *cur[3], *next[3];     // Y, Cb, Cr of P, C and N (they may be the same planes: the first and the last frame of a clip)
    void *dst[3];                               // coded-size planes; 16-byte aligned, strides too
    int pitch[3];                               // of every source frame, in elements
    int dstride[3];                             // in samples
    int align[3];                               // per plane: the narrowest class of the three frames (ingest_align)
    int w, h, pw, ph;                           // display and coded size of luma
    int keep, second, vmax;
};

HDI bool deint_geometry_ok(int w, int h) { return w >= 16 && h >= 16 && !(w & 1) && !(h & 3); }
HDI bool deint_mode_ok(const mihevc_deint *d)
{
    if (!d || (d->tff != 0 && d->tff != 1) || (d->field_rate != 0 && d->field_rate != 1)) return false;
    return !(d->reserved[0] | d->reserved[1] | d->reserved[2] | d->reserved[3] | d->reserved[4] | d->reserved[5]);
}
HDI int deint_tiles(int w, int h) { return ((w + DI_TW - 1) / DI_TW) * ((h + DI_TH - 1) / DI_TH); }
HDI int deint_workgroups(int pw, int ph) { return deint_tiles(pw, ph) + 2 * deint_tiles(pw / 2, ph / 2); }
// workgroup r -> component (0 Y, 1 Cb, 2 Cr), r becomes the tile inside it; -1 past the last
HDI int deint_locate(int pw, int ph, int &r)
{
    const int ny = deint_tiles(pw, ph), nc = deint_tiles(pw / 2, ph / 2);
    if (r < ny) return 0;
    r -= ny;
    if (r < nc) return 1;
    r -= nc;
    return r < nc ? 2 : -1;
}
// every field from the geometry and the planes.  prev / cur / next: Y, Cb, Cr of the three frames, one pitch_y and one pitch_c for all of them
inline DeintArgs deint_args(int depth, const void *const *prev, const void *const *cur, const void *const *next, int pitch_y, int pitch_c, int w, int h, int pw, int ph,
                            int keep, int second, void *const *out, const int *ostride)
{
    DeintArgs a;
    const size_t es = depth > 8 ? 2 : 1;
    for (int c = 0; c < 3; c++) {
        a.prev[c] = prev[c]; a.cur[c] = cur[c]; a.next[c] = next[c]; a.dst[c] = out[c]; a.dstride[c] = ostride[c]; a.pitch[c] = c ? pitch_c : pitch_y;
        const size_t pb = (size_t)a.pitch[c] * es;
        const int al0 = ingest_align(prev[c], pb), al1 = ingest_align(cur[c], pb), al2 = ingest_align(next[c], pb);
        a.align[c] = al0 < al1 ? (al0 < al2 ? al0 : al2) : (al1 < al2 ? al1 : al2);
    }
    a.w = w; a.h = h; a.pw = pw; a.ph = ph; a.keep = keep; a.second = second; a.vmax = (1 << depth) - 1;
    return a;
}

// the row that stands for row r of a plane hh rows high (-2 <= r <= hh + 1, hh >= 4)
DEV int deint_row(int r, int hh) { return r < 0 ? r + 2 : r >= hh ? r - 2 : r; }
// the run at columns x0 .. x0 + ING_RUN - 1 of one row, values clamped; a run that reaches past ww: its elements at clamped columns
template <typename TI> DEV void deint_run(const TI *row, int x0, int ww, int al, int vmax, int (&v)[ING_RUN])
{
    if (x0 >= 0 && x0 + ING_RUN <= ww) ingest_load<TI, ING_RUN>(row + x0, al, v);
    else {
#pragma unroll
        for (int k = 0; k < ING_RUN; k++) ingest_element(row + clip3(0, ww - 1, x0 + k), v[k]);
    }
#pragma unroll
    for (int k = 0; k < ING_RUN; k++) v[k] = imin(v[k], vmax);
}
// ING_RUN samples of the LDS image from p (16-byte aligned)
DEV void deint_lds_run(const uint16_t *p, int *v)
{
    const ingest_u32x4 w = *(const ingest_u32x4 *)__builtin_assume_aligned(p, 16);
#pragma unroll
    for (int k = 0; k < ING_RUN / 2; k++) { v[2 * k] = (int)(w[k] & 0xffffu); v[2 * k + 1] = (int)(w[k] >> 16); }
}

// the missing row ye of the lane's run: up / dn are C[ye-1] / C[ye+1] at columns x0 - ING_RUN .. x0 + 2 ING_RUN - 1; the others at x0 .. x0 + ING_RUN - 1
DEV void deint_filter(const int (&up)[3 * ING_RUN], const int (&dn)[3 * ING_RUN], const int (&c0)[ING_RUN], const int (&cm2)[ING_RUN], const int (&cp2)[ING_RUN],
                      const int (&x0v)[ING_RUN], const int (&xm2)[ING_RUN], const int (&xp2)[ING_RUN], const int (&pm)[ING_RUN], const int (&pp)[ING_RUN],
                      const int (&nm)[ING_RUN], const int (&np)[ING_RUN], int (&o)[ING_RUN])
{
#pragma unroll
    for (int k = 0; k < ING_RUN; k++) {
        const int i = k + ING_RUN, c = up[i], e = dn[i];
        const int d = (x0v[k] + c0[k]) >> 1;
        int diff = imax(imax(iabs(x0v[k] - c0[k]) >> 1, (iabs(pm[k] - c) + iabs(pp[k] - e)) >> 1), (iabs(nm[k] - c) + iabs(np[k] - e)) >> 1);
        auto score = [&](int j) { return iabs(up[i - 1 + j] - dn[i - 1 - j]) + iabs(up[i + j] - dn[i - j]) + iabs(up[i + 1 + j] - dn[i + 1 - j]); };
        auto pred = [&](int j) { return (up[i + j] + dn[i - j]) >> 1; };
        int best = score(0) - 1, sp = pred(0);
        if (score(-1) < best) {
            best = score(-1); sp = pred(-1);
            if (score(-2) < best) { best = score(-2); sp = pred(-2); }
        }
        if (score(1) < best) {
            best = score(1); sp = pred(1);
            if (score(2) < best) { best = score(2); sp = pred(2); }
        }
        const int b = (xm2[k] + cm2[k]) >> 1, f = (xp2[k] + cp2[k]) >> 1;
        const int mx = imax(imax(d - e, d - c), imin(b - c, f - e)), mn = imin(imin(d - e, d - c), imax(b - c, f - e));
        diff = imax(imax(diff, mn), -mx);
        o[k] = sp > d + diff ? d + diff : sp < d - diff ? d - diff : sp;
    }
}

// workgroup `wg` of the launch
template <typename T, class Ex> DEV void deint_tile_program(Ex &ex, DeintShared &s, const DeintArgs &a, int wg)
{
    int tile = wg;
    const int c = deint_locate(a.pw, a.ph, tile);
    if (c < 0) return;
    const T *const P = (const T *)a.prev[c], *const C = (const T *)a.cur[c], *const N = (const T *)a.next[c], *const X = a.second ? N : P;
    T *const dst = (T *)a.dst[c];
    const int pitch = a.pitch[c], dstride = a.dstride[c], al = a.align[c], keep = a.keep, vmax = a.vmax;
    const int ww = c ? a.w / 2 : a.w, hh = c ? a.h / 2 : a.h, pwo = c ? a.pw / 2 : a.pw, pho = c ? a.ph / 2 : a.ph;
    const int ntx = (pwo + DI_TW - 1) / DI_TW, ty = tile / ntx, tx = tile - ty * ntx;
    const int xl = tx * DI_TW - ING_RUN, yl = ty * DI_TH - 2;            // column and row of the image's first sample
    ex.phase([&](int tid) {          // the image of C: run q % DI_RUNS of row q / DI_RUNS
        for (int q = tid; q < DI_LH * DI_RUNS; q += NT) {
            const int l = q / DI_RUNS, rn = q - l * DI_RUNS, x0 = xl + rn * ING_RUN, r = yl + l;
            if (x0 >= pwo + ING_RUN || r > hh + 1) continue;             // no lane of phase 2 reads it
            int v[ING_RUN];
            deint_run<T>(C + (ptrdiff_t)deint_row(r, hh) * pitch, x0, ww, al, vmax, v);
            *(ingest_u32x4 *)__builtin_assume_aligned(&s.c[l][rn * ING_RUN], 16) =
                ingest_u32x4{(uint32_t)v[0] | (uint32_t)v[1] << 16, (uint32_t)v[2] | (uint32_t)v[3] << 16, (uint32_t)v[4] | (uint32_t)v[5] << 16, (uint32_t)v[6] | (uint32_t)v[7] << 16};
        }
    });
    ex.phase([&](int tid) {          // the lane's run of rows y and y + 1: one of them kept, the other filtered
        const int lx = tid & (DI_LX - 1), ly = tid / DI_LX, x0 = tx * DI_TW + lx * ING_RUN;
        if (x0 >= pwo) return;
        const int last = ww - 1 - x0;                                    // the run's last sample inside the display area (>= 0)
        for (int i = 0; i < 2; i++) {
            const int y = ty * DI_TH + 2 * ly + i;
            if (y >= pho) return;
            const int ye = imin(y, hh - 1), l = ye - yl;
            int o[ING_RUN];
            if ((ye & 1) == keep) deint_lds_run(&s.c[l][(lx + 1) * ING_RUN], o);
            else {
                int pm[ING_RUN], pp[ING_RUN], nm[ING_RUN], np[ING_RUN], x0v[ING_RUN], xm2[ING_RUN], xp2[ING_RUN];
                const ptrdiff_t rm1 = (ptrdiff_t)deint_row(ye - 1, hh) * pitch, rp1 = (ptrdiff_t)deint_row(ye + 1, hh) * pitch;
                deint_run<T>(P + rm1, x0, ww, al, vmax, pm);
                deint_run<T>(P + rp1, x0, ww, al, vmax, pp);
                deint_run<T>(N + rm1, x0, ww, al, vmax, nm);
                deint_run<T>(N + rp1, x0, ww, al, vmax, np);
                deint_run<T>(X + (ptrdiff_t)ye * pitch, x0, ww, al, vmax, x0v);
                deint_run<T>(X + (ptrdiff_t)deint_row(ye - 2, hh) * pitch, x0, ww, al, vmax, xm2);
                deint_run<T>(X + (ptrdiff_t)deint_row(ye + 2, hh) * pitch, x0, ww, al, vmax, xp2);
                int up[3 * ING_RUN], dn[3 * ING_RUN], c0[ING_RUN], cm2[ING_RUN], cp2[ING_RUN];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    deint_lds_run(&s.c[l - 1][(lx + k) * ING_RUN], up + k * ING_RUN);
                    deint_lds_run(&s.c[l + 1][(lx + k) * ING_RUN], dn + k * ING_RUN);
                }
                deint_lds_run(&s.c[l][(lx + 1) * ING_RUN], c0);
                deint_lds_run(&s.c[l - 2][(lx + 1) * ING_RUN], cm2);
                deint_lds_run(&s.c[l + 2][(lx + 1) * ING_RUN], cp2);
                deint_filter(up, dn, c0, cm2, cp2, x0v, xm2, xp2, pm, pp, nm, np, o);
#pragma unroll
                for (int k = 1; k < ING_RUN; k++) o[k] = k > last ? o[k - 1] : o[k];      // the margin's columns repeat the last one inside
            }
            ingest_store(dst + (ptrdiff_t)y * dstride + x0, o, x0 + ING_RUN <= pwo);
        }
    });
}

}  // namespace mihevc
