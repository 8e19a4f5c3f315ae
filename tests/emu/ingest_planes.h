// tests/emu/ingest_planes.h — TEST HARNESS, NOT PRODUCT.  What the stepped source converters (tests/emu/ingest.cpp, tests/emu/ingest_rgb.cpp) share: the one
// definition of the kernel headers' access hook with its counter, and the planes a run works on.  Include it before the kernel header.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

// the kernel headers' access hook: loads and stores whose address is not a multiple of their width.  One counter and one definition for the whole library, so
// every inline function of the headers has one body in it; a run resets the counter first
inline int g_ingest_misaligned = 0;
#define MIHEVC_INGEST_ACCESS(p, bytes) ((void)(g_ingest_misaligned += ((uintptr_t)(p) % (unsigned)(bytes)) != 0))

// A source plane of alignment class `align`, filled from the caller's tight rows.  align 16, 8, 4: the base address and the pitch in bytes are multiples of it
// and of nothing larger; 1: base one element off, odd pitch.  The allocation ends with the last sample of the last row, and the pitch is wider than the row
template <typename TI> struct IngestSrcPlane {
    void *base = nullptr;
    const TI *p = nullptr;
    int pitch = 0;      // elements
    IngestSrcPlane() = default;
    IngestSrcPlane(const IngestSrcPlane &) = delete;
    ~IngestSrcPlane() { free(base); }
    bool place(const void *tight, int row, int rows, int align)
    {
        const int unit = align > (int)sizeof(TI) ? align / (int)sizeof(TI) : 1;             // elements
        pitch = ((row + unit - 1) / unit + 1) * unit;
        if (align < 16 && (pitch / unit) % 2 == 0) pitch += unit;                           // an odd multiple: not a multiple of the next power of two
        const size_t off = align == 16 ? 0 : align == 1 ? sizeof(TI) : (size_t)align;       // bytes from a 64-byte boundary
        const size_t bytes = ((size_t)pitch * (rows - 1) + row) * sizeof(TI);
        if (posix_memalign(&base, 64, off + bytes)) return false;
        memset(base, 0x5A, off + bytes);
        TI *q = (TI *)((uint8_t *)base + off);
        for (int r = 0; r < rows; r++) memcpy(q + (size_t)r * pitch, (const TI *)tight + (size_t)r * row, (size_t)row * sizeof(TI));
        p = q;
        return true;
    }
};

// The three output planes of the coded size pw x ph (4:2:0), their strides wider than the coded width and every sample a garbage pattern, so an unwritten
// sample shows and the samples between the coded width and the stride must still hold the pattern afterwards
template <typename TO> struct IngestOutPlanes {
    static constexpr TO kGarbage = (TO)0xA5A5;
    void *dst[3];
    int stride[3], w[3], h[3];
    IngestOutPlanes(int pw, int ph)
    {
        for (int c = 0; c < 3; c++) {
            w[c] = c ? pw / 2 : pw; h[c] = c ? ph / 2 : ph;
            stride[c] = ((w[c] + 15) & ~15) + 16;
            dst[c] = aligned_alloc(64, ((size_t)stride[c] * h[c] * sizeof(TO) + 63) & ~(size_t)63);
            for (size_t i = 0; i < (size_t)stride[c] * h[c]; i++) ((TO *)dst[c])[i] = kGarbage;
        }
    }
    IngestOutPlanes(const IngestOutPlanes &) = delete;
    ~IngestOutPlanes() { for (void *d : dst) free(d); }
    // the planes to the caller's tight ones; returns the number of samples written past the coded width
    int copy_back(void *const *out) const
    {
        int spilled = 0;
        for (int c = 0; c < 3; c++)
            for (int r = 0; r < h[c]; r++) {
                const TO *row = (const TO *)dst[c] + (size_t)r * stride[c];
                memcpy((TO *)out[c] + (size_t)r * w[c], row, (size_t)w[c] * sizeof(TO));
                for (int x = w[c]; x < stride[c]; x++) spilled += row[x] != kGarbage;
            }
        return spilled;
    }
};
