// hevc_amd/csrc/md5.h — MD5 (RFC 1321) for the decoded picture hash SEI (hash_type 0): host code, written from the RFC.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace mihevc {

class Md5 {
public:
    Md5() { h_[0] = 0x67452301u; h_[1] = 0xefcdab89u; h_[2] = 0x98badcfeu; h_[3] = 0x10325476u; }
    void update(const uint8_t *p, size_t n)
    {
        len_ += n;
        if (fill_) {
            const size_t k = n < 64 - fill_ ? n : 64 - fill_;
            memcpy(buf_ + fill_, p, k);
            fill_ += k; p += k; n -= k;
            if (fill_ < 64) return;
            block(buf_);
            fill_ = 0;
        }
        for (; n >= 64; p += 64, n -= 64) block(p);
        memcpy(buf_, p, n);
        fill_ = n;
    }
    // padding: 0x80, zeros up to 56 mod 64, the message length in bits (64-bit little endian); digest = A B C D little endian
    void final(uint8_t out[16])
    {
        const uint64_t bits = (uint64_t)len_ * 8;
        uint8_t pad[72] = {0x80};
        const size_t np = fill_ < 56 ? 56 - fill_ : 120 - fill_;
        for (int i = 0; i < 8; i++) pad[np + i] = (uint8_t)(bits >> (8 * i));
        update(pad, np + 8);
        for (int i = 0; i < 16; i++) out[i] = (uint8_t)(h_[i >> 2] >> (8 * (i & 3)));
    }

private:
    uint32_t h_[4];
    uint8_t buf_[64];
    size_t fill_ = 0;
    uint64_t len_ = 0;

    static uint32_t rotl(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }
    // T[i] = floor(2^32 |sin(i + 1)|) (RFC 1321 3.4)
    static const uint32_t *table()
    {
        static const struct T { uint32_t k[64]; T() { for (int i = 0; i < 64; i++) k[i] = (uint32_t)std::floor(4294967296.0 * std::fabs(std::sin((double)(i + 1)))); } } t;
        return t.k;
    }
    void block(const uint8_t *p)
    {
        static const int S[4][4] = {{7, 12, 17, 22}, {5, 9, 14, 20}, {4, 11, 16, 23}, {6, 10, 15, 21}};
        const uint32_t *K = table();
        uint32_t m[16];
        for (int i = 0; i < 16; i++) m[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
        uint32_t a = h_[0], b = h_[1], c = h_[2], d = h_[3];
        for (int i = 0; i < 64; i++) {
            uint32_t f;
            int g;
            if (i < 16) { f = (b & c) | (~b & d); g = i; }
            else if (i < 32) { f = (d & b) | (~d & c); g = (5 * i + 1) & 15; }
            else if (i < 48) { f = b ^ c ^ d; g = (3 * i + 5) & 15; }
            else { f = c ^ (b | ~d); g = (7 * i) & 15; }
            const uint32_t t = d;
            d = c;
            c = b;
            b = b + rotl(a + f + K[i] + m[g], S[i >> 4][i & 3]);
            a = t;
        }
        h_[0] += a; h_[1] += b; h_[2] += c; h_[3] += d;
    }
};

// MD5 of one component's pictureData: `rows` rows of `row_bytes` bytes, `pitch` bytes apart (the bytes of a row are its samples as they lie in memory:
// one byte each at 8 bit, low byte first above 8 bit)
inline void md5_plane(const uint8_t *p, size_t pitch, size_t row_bytes, int rows, uint8_t out[16])
{
    Md5 m;
    for (int y = 0; y < rows; y++) m.update(p + (size_t)y * pitch, row_bytes);
    m.final(out);
}

}  // namespace mihevc
