// tests/emu/pichash.cpp — TEST HARNESS, NOT PRODUCT (part of tests/emu/libkernel_emu.so).  The decoded picture hash programs of hevc_amd/csrc/kernels/pichash.h (k_pic_hash, then
// k_pic_hash_fold) stepped on the CPU with the sequential executor, over host planes laid out as mihevc_k_picture_hash takes them; the planes sit in a
// border as a session's final reconstruction does, so rows are hashed through a pitch.  hevc_amd/ never loads this library.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hevc_amd/csrc/kernels/pichash.h"

using namespace mihevc;

extern "C" {

// kind 1 CRC, 2 checksum; order: SeqExec thread order (0 ascending, 1 descending, 2 random per phase); out: three hash words.  Returns 0, or -3
int emu_picture_hash(const void *y, const void *u, const void *v, int w, int h, int bit_depth, int kind, int order, uint32_t *out)
{
    if (w < 8 || h < 8 || (w & 7) || (h & 7) || (bit_depth != 8 && bit_depth != 10) || (kind != 1 && kind != 2)) return -3;
    const int bps = bit_depth > 8 ? 2 : 1;
    const void *src[3] = {y, u, v};
    std::vector<std::vector<uint8_t>> store(3);
    HashPlane pl[3];
    for (int c = 0; c < 3; c++) {
        const int pw = c ? w / 2 : w, ph = c ? h / 2 : h, pad = c ? 40 : 80;
        const size_t pitch = (size_t)((pw + 2 * pad + 63) & ~63) * bps;
        store[c].assign(pitch * (ph + 2 * pad), 0xA5);       // a border that is not part of the picture
        uint8_t *p = store[c].data() + pitch * pad + (size_t)pad * bps;
        for (int r = 0; r < ph; r++) memcpy(p + pitch * r, (const uint8_t *)src[c] + (size_t)r * pw * bps, (size_t)pw * bps);
        pl[c] = HashPlane{p, (long long)pitch, pw * bps / 4, ph};
    }
    SeqExec ex;
    ex.order = order;
    const int nb_y = hash_blocks(pl[0]), nb_c = hash_blocks(pl[1]), nb = nb_y + 2 * nb_c;
    std::vector<uint32_t> part((size_t)nb, 0xDEADBEEFu);
    PicHashShared *s = (PicHashShared *)malloc(sizeof(PicHashShared));
    for (int b = 0; b < nb; b++) {                           // k_pic_hash: one workgroup per segment
        memset(s, 0x5A, sizeof *s);                          // LDS holds garbage at workgroup start
        int blk = b;
        const int c = hash_locate(nb_y, nb_c, blk);
        pichash_block_program(ex, *s, pl[c], bps, kind, blk, &part[(size_t)b]);
    }
    for (int c = 0; c < 3; c++) {                            // k_pic_hash_fold: one workgroup per component
        memset(s, 0x5A, sizeof *s);
        pichash_fold_program(ex, *s, pl[c], kind, part.data() + hash_first_block(nb_y, nb_c, c), out + c);
    }
    free(s);
    return 0;
}

}  // extern "C"
