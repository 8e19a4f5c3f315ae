// hevc_amd/csrc/kernels/pichash.h — decoded picture hash (H.265 Annex D, SEI payloadType 132; x265 --hash): CRC and checksum of the final
// reconstruction over the CODED size, per colour component.
//
// pictureData of a component is its samples in raster order, one byte each at 8 bit, low byte then high byte above 8 bit: exactly the bytes of
// each row as they lie in memory.  Coded widths are multiples of 8, so every row is a whole number of dwords and the byte stream is hashed a
// dword at a time.  Two launches per step, each covering every picture of the batch and all three components:
//   k_pic_hash       one workgroup per HASH_SEG dwords of a component's stream; lane l takes dwords d0 + l, d0 + l + NT, ... (one coalesced
//                    dword load per lane and iteration) and leaves one partial per workgroup in a scratch array
//   k_pic_hash_fold  one workgroup per (picture, component): the partials in stream order -> the hash word
// CRC (hash_type 1): the register of the Annex D bit loop after the bits b_0 .. b_{n-1} is (R0 x^n + sum b_i x^{n-1-i}) mod P, P = x^16 + x^12 +
// x^5 + 1: linear over GF(2).  A workgroup's partial is the zero-initialised remainder of its segment, M_seg(x) mod P; segments combine as
// r = r_left x^(8 len_right) + r_right.  Inside a workgroup each lane runs Horner over its strided dwords (the stride is a multiplication by a
// constant, two 256-entry LDS tables) and then shifts its remainder to the segment's end: the lanes' terms are disjoint, the XOR of all of them
// is the segment's remainder.  The fold does the same with the segments, then the affine part: crc = ((0xFFFF x^(8L) + r) x^16) mod P for L
// data bytes (start value 0xFFFF, two zero bytes appended).  Every combine is XOR: the result does not depend on the order anything ran in.
// Checksum (hash_type 2): sum over samples of (s & 0xFF) ^ mask (+ (s >> 8) ^ mask above 8 bit), mask = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8),
// modulo 2^32: uint32 partials per lane, summed per workgroup and then per component; integer sums are order-independent too.
// MD5 (hash_type 0) is computed on the host (csrc/md5.h).
#pragma once
#include "common.h"

namespace mihevc {

constexpr int HASH_K = 32;                  // dwords per lane and workgroup
constexpr int HASH_SEG = NT * HASH_K;       // dwords of a component's stream per workgroup (32 KB)
constexpr uint32_t CRC_POLY = 0x1021;       // P(x) without its x^16 term; also x^16 mod P

// GF(2)[x] modulo P on 16-bit remainders
constexpr uint32_t crc_xtime(uint32_t r) { return ((r << 1) & 0xffffu) ^ (((r >> 15) & 1u) ? CRC_POLY : 0u); }
constexpr uint32_t crc_mulmod(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r = crc_xtime(r);
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}
struct CrcPow { uint16_t p[32]; };          // p[i] = x^(8 * 2^i) mod P
constexpr CrcPow make_crc_pow()
{
    CrcPow t{};
    uint32_t v = 1;
    for (int k = 0; k < 8; k++) v = crc_xtime(v);
    for (int i = 0; i < 32; i++) { t.p[i] = (uint16_t)v; v = crc_mulmod(v, v); }
    return t;
}
DEVCONST CrcPow g_crc_pow = make_crc_pow();
// x^(8 n) mod P: the shift of a remainder past n bytes
DEV uint32_t crc_xpow8(uint32_t n)
{
    uint32_t r = 1;
    for (int i = 0; n; i++, n >>= 1)
        if (n & 1u) r = crc_mulmod(r, g_crc_pow.p[i]);
    return r;
}
constexpr uint32_t crc_xpow8_const(uint32_t n)
{
    uint32_t r = 1;
    for (uint32_t k = 0; k < 8 * n; k++) r = crc_xtime(r);
    return r;
}
// what Horner multiplies by between a lane's consecutive dwords (NT dwords apart) before the 4 new bytes are shifted in
constexpr uint32_t kCrcStride = crc_xpow8_const(4 * (NT - 1));

// one component of one picture: `rows` rows of `row_dwords` dwords, `pitch` bytes apart
struct HashPlane {
    const uint8_t *p;
    long long pitch;
    int row_dwords, rows;
};
HDI int hash_dwords(const HashPlane &q) { return q.row_dwords * q.rows; }
HDI int hash_blocks(const HashPlane &q) { return (hash_dwords(q) + HASH_SEG - 1) / HASH_SEG; }
// The workgroups of a picture cover Y, then Cb, then Cr (nb_y / nb_c blocks each; both chroma components have the same size).
// workgroup b -> component, b becomes the block inside it; -1 past the last
HDI int hash_locate(int nb_y, int nb_c, int &b)
{
    if (b < nb_y) return 0;
    b -= nb_y;
    if (b < 2 * nb_c) { const int c = 1 + b / nb_c; b -= (c - 1) * nb_c; return c; }
    return -1;
}
HDI int hash_first_block(int nb_y, int nb_c, int c) { return c ? nb_y + (c - 1) * nb_c : 0; }

struct PicHashShared {
    uint16_t tab[256];      // b x^16 mod P: one byte shifted through the register
    uint16_t mlo[256];      // b kCrcStride mod P
    uint16_t mhi[256];      // b x^8 kCrcStride mod P
    uint32_t red[NT];
};

// 256 remainders -> red[0]: four per lane of the first wave, then halving steps inside that wave (XOR for the CRC, + for the checksum)
template <class Ex> DEV void hash_reduce(Ex &ex, PicHashShared &s, bool crc)
{
    ex.wave_step([&](int tid) {
        if (tid >= 64) return;
        const uint32_t a = s.red[tid], b = s.red[tid + 64], c = s.red[tid + 128], d = s.red[tid + 192];
        s.red[tid] = crc ? a ^ b ^ c ^ d : a + b + c + d;
    });
    for (int h = 32; h > 0; h >>= 1)
        ex.wave_step([&](int tid) {
            if (tid < h) s.red[tid] = crc ? s.red[tid] ^ s.red[tid + h] : s.red[tid] + s.red[tid + h];
        });
}

// segment `blk` of component q (bps bytes per sample): its partial -> *part.  kind 1 CRC, 2 checksum
template <class Ex> DEV void pichash_block_program(Ex &ex, PicHashShared &s, const HashPlane &q, int bps, int kind, int blk, uint32_t *part)
{
    const int n = hash_dwords(q), d0 = blk * HASH_SEG, d1 = imin(n, d0 + HASH_SEG), rd = q.row_dwords;
    const bool crc = kind == 1;
    if (crc)
        ex.phase([&](int tid) {
            uint32_t t = (uint32_t)tid << 8;      // tid x^8 -> x^16 by eight shifts
            for (int k = 0; k < 8; k++) t = crc_xtime(t);
            s.tab[tid] = (uint16_t)t;
            s.mlo[tid] = (uint16_t)crc_mulmod((uint32_t)tid, kCrcStride);
            s.mhi[tid] = (uint16_t)crc_mulmod((uint32_t)tid << 8, kCrcStride);
        });
    ex.phase([&](int tid) {
        const int rstep = NT / rd, cstep = NT % rd;
        int d = d0 + tid, row = d / rd, col = d - row * rd, last = -1;
        uint32_t acc = 0;
        for (; d < d1; d += NT) {
            const uint32_t v = load_u32(q.p + (long long)row * q.pitch + 4 * col);
            if (crc) {
                acc = (uint32_t)s.mhi[acc >> 8] ^ s.mlo[acc & 255];
#pragma unroll
                for (int k = 0; k < 4; k++) acc = (uint32_t)s.tab[acc >> 8] ^ ((acc & 255) << 8) ^ ((v >> (8 * k)) & 255);
            } else {
                const uint32_t ym = (uint32_t)(row & 255) ^ (uint32_t)(row >> 8);
                if (bps == 1) {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int x = 4 * col + k;
                        acc += ((v >> (8 * k)) & 255) ^ (ym ^ (uint32_t)(x & 255) ^ (uint32_t)(x >> 8));
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        const int x = 2 * col + k;
                        const uint32_t m = ym ^ (uint32_t)(x & 255) ^ (uint32_t)(x >> 8), smp = (v >> (16 * k)) & 0xffffu;
                        acc += ((smp & 255) ^ m) + ((smp >> 8) ^ m);
                    }
                }
            }
            last = d;
            row += rstep; col += cstep;
            if (col >= rd) { col -= rd; row++; }
        }
        if (crc && last >= 0) acc = crc_mulmod(acc, crc_xpow8(4u * (uint32_t)(d1 - 1 - last)));      // to the end of the segment
        s.red[tid] = acc;
    });
    hash_reduce(ex, s, crc);
    ex.wave_step([&](int tid) { if (tid == 0) *part = s.red[0]; });
}

// component q: its segments' partials part[0 .. nb) in stream order -> *out
template <class Ex> DEV void pichash_fold_program(Ex &ex, PicHashShared &s, const HashPlane &q, int kind, const uint32_t *part, uint32_t *out)
{
    const int n = hash_dwords(q), nb = hash_blocks(q);
    const bool crc = kind == 1;
    ex.phase([&](int tid) {
        const int b0 = (int)((long long)nb * tid / NT), b1 = (int)((long long)nb * (tid + 1) / NT);      // a run of consecutive segments
        uint32_t acc = 0;
        for (int b = b0; b < b1; b++) {
            const uint32_t v = part[b];
            if (crc) acc = crc_mulmod(acc, crc_xpow8(4u * (uint32_t)(imin(n, (b + 1) * HASH_SEG) - b * HASH_SEG))) ^ v;
            else acc += v;
        }
        if (crc && b1 > b0) acc = crc_mulmod(acc, crc_xpow8(4u * (uint32_t)(n - imin(n, b1 * HASH_SEG))));      // to the end of the stream
        s.red[tid] = acc;
    });
    hash_reduce(ex, s, crc);
    ex.wave_step([&](int tid) {
        if (tid) return;
        *out = crc ? crc_mulmod(crc_mulmod(0xffffu, crc_xpow8(4u * (uint32_t)n)) ^ s.red[0], CRC_POLY) : s.red[0];
    });
}

}  // namespace mihevc
