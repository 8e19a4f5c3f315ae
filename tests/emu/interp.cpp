// tests/emu/interp.cpp — TEST HARNESS, NOT PRODUCT (part of tests/emu/libkernel_emu.so).  The fractional-sample interpolation of
// hevc_amd/csrc/kernels/inter.h called directly on a caller's window: the sample primitives of motion compensation (luma_quad14, chroma_sample14,
// weighted_uni), the fractional search's luma_half_diff, and the LDS layouts of the two
// CTU kernels (tests/test_interp_cpu.py).  hevc_amd/ never loads this library.
#include "../../hevc_amd/csrc/kernels/inter.h"

using namespace mihevc;

namespace {

// `win`: a 4-byte aligned window image with row stride ws; i00: the element index of the block's first integer sample
template <typename T> void luma14(const T *win, int i00, int ws, int bd, int *out)
{
    for (int f = 0; f < 16; f++)
        for (int j = 0; j < 8; j++) {
            int v[4];
            luma_quad14<T>(win, i00 + j * ws, ws, f & 3, f >> 2, bd, v);
            for (int i = 0; i < 4; i++) out[(f * 8 + j) * 4 + i] = v[i];
        }
}
template <typename T> void chroma14(const T *win, int i00, int ws, int bd, int *out)
{
    for (int f = 0; f < 64; f++)
        for (int j = 0; j < 4; j++)
            for (int i = 0; i < 4; i++) out[(f * 4 + j) * 4 + i] = chroma_sample14<T>(win + i00 + j * ws + i, ws, f & 7, f >> 3, bd);
}
template <typename T> void half_diff(const T *win, int i00, int ws, int bd, const T *src, int src_stride, int mixed_wave, int *out)
{
    struct Mixed { Mixed(bool on) { g_emu_mixed_wave = on; } ~Mixed() { g_emu_mixed_wave = false; } } mixed(mixed_wave != 0);
    for (int f = 0; f < 16; f++) {
        int m[8][4];
        luma_half_diff(win, i00, ws, f & 3, f >> 2, bd, src, src_stride, m);
        for (int j = 0; j < 8; j++)
            for (int i = 0; i < 4; i++) out[(f * 8 + j) * 4 + i] = m[j][i];
    }
}
template <typename T> void layout(int R, long long *o)
{
    const InterLds p = inter_lds<T>(R);
    const InterBLds b = inter_b_lds<T>(R);
    const long long v[13] = {(long long)mc_win_y_bytes<T>(R), (long long)mc_win_c_bytes<T>(R), (long long)p.y, (long long)p.u, (long long)p.v, (long long)p.bytes,
                             p.y == inter_win_in<T>(), (long long)b.y, (long long)b.u, (long long)b.v, (long long)b.bi, (long long)b.bytes, mc_win_y_stride(R)};
    for (int i = 0; i < 13; i++) o[i] = v[i];
}

}  // namespace

extern "C" {

// the 14-bit predictions of the 8 rows x 4 columns (luma) / 4 x 4 samples (chroma) at i00 for every fraction f = fy * 4 + fx (chroma: fy * 8 + fx):
// out[f][row][column]; the window holds uint8 samples at 8 bit, uint16 at 10
void emu_interp_luma14(const void *win, int i00, int ws, int bd, int *out)
{
    bd == 8 ? luma14((const uint8_t *)win, i00, ws, bd, out) : luma14((const uint16_t *)win, i00, ws, bd, out);
}
void emu_interp_chroma14(const void *win, int i00, int ws, int bd, int *out)
{
    bd == 8 ? chroma14((const uint8_t *)win, i00, ws, bd, out) : chroma14((const uint16_t *)win, i00, ws, bd, out);
}
int emu_weighted_uni(int p, int bd) { return weighted_uni(p, bd); }
// source - prediction of the same block as the fractional search takes it (luma_half_diff), for every fraction.  mixed_wave: as a lane of a wave whose
// lanes disagree on every wave_all (common.h g_emu_mixed_wave): the general two-pass path for zero fractions too, instead of the one-pass paths
void emu_interp_half_diff(const void *win, int i00, int ws, int bd, const void *src, int src_stride, int mixed_wave, int *out)
{
    bd == 8 ? half_diff((const uint8_t *)win, i00, ws, bd, (const uint8_t *)src, src_stride, mixed_wave, out)
            : half_diff((const uint16_t *)win, i00, ws, bd, (const uint16_t *)src, src_stride, mixed_wave, out);
}
// sample_bytes 1 / 2, me_range R: window bytes (luma, chroma); k_inter_ctu: offsets of the three windows, dynamic LDS, luma window inside rs.scratch;
// k_inter_ctu_b: offsets of the three windows and of BiShared, dynamic LDS; the luma window's row stride
void emu_inter_layout(int sample_bytes, int R, long long *out13) { sample_bytes == 1 ? layout<uint8_t>(R, out13) : layout<uint16_t>(R, out13); }

}  // extern "C"
