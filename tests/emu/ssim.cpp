// tests/emu/ssim.cpp — TEST HARNESS, NOT PRODUCT (part of tests/emu/libkernel_emu.so).  The SSIM programs of hevc_amd/csrc/kernels/ssim.h (k_ssim, then k_ssim_fold)
// stepped on the CPU with the sequential executor, over host planes laid out as mihevc_k_ssim takes them.  The source sits in a plain pitched plane and the
// reconstruction in a border, as in a session; every plane is allocated to its exact size, so a read past it is a finding of the sanitizer build
// (tests/sanitize_cpu.sh).  hevc_amd/ never loads this library.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hevc_amd/csrc/kernels/ssim.h"

using namespace mihevc;

namespace {

template <typename T> int run(const void *const *a, const void *const *b, int w, int h, int order, long long *sum, long long *windows)
{
    std::vector<std::vector<T>> sa(3), sb(3);
    SsimPlane<T> pl[3];
    for (int c = 0; c < 3; c++) {
        const int pw = c ? w / 2 : w, ph = c ? h / 2 : h, pad = c ? PAD_C : PAD_Y;
        const int pitch_a = (pw + 63) & ~63, pitch_b = (pw + 2 * pad + 63) & ~63;
        sa[c].assign((size_t)pitch_a * (ph - 1) + pw, (T)0xA5);                           // ends with the last sample of the last row
        sb[c].assign((size_t)pitch_b * (ph + 2 * pad), (T)0xA5);                          // a border that is not part of the picture
        T *pb = sb[c].data() + (size_t)pitch_b * pad + pad;
        for (int r = 0; r < ph; r++) {
            memcpy(sa[c].data() + (size_t)pitch_a * r, (const T *)a[c] + (size_t)r * pw, (size_t)pw * sizeof(T));
            memcpy(pb + (size_t)pitch_b * r, (const T *)b[c] + (size_t)r * pw, (size_t)pw * sizeof(T));
        }
        pl[c] = SsimPlane<T>{sa[c].data(), pb, pitch_a, pitch_b, pw, ph};
        windows[c] = (long long)ssim_windows_x(pw) * ssim_windows_y(ph);
    }
    SeqExec ex;
    ex.order = order;
    const int nr_y = ssim_regions(pl[0].w, pl[0].h), nr_c = ssim_regions(pl[1].w, pl[1].h), nr = nr_y + 2 * nr_c;
    std::vector<long long> part((size_t)nr, 0x5EADBEEF5EADBEEFll);
    SsimShared *s = (SsimShared *)malloc(sizeof(SsimShared));
    for (int r = 0; r < nr; r++) {                           // k_ssim: one workgroup per region
        memset(s, 0x5A, sizeof *s);                          // LDS holds garbage at workgroup start
        int reg = r;
        const int c = ssim_locate(nr_y, nr_c, reg);
        ssim_region_program<T>(ex, *s, pl[c], reg, &part[(size_t)r]);
    }
    for (int c = 0; c < 3; c++) {                            // k_ssim_fold: one workgroup per component
        memset(s, 0x5A, sizeof *s);
        ssim_fold_program(ex, *s, c ? nr_c : nr_y, part.data() + ssim_first_region(nr_y, nr_c, c), sum + c);
    }
    free(s);
    return 0;
}

}  // namespace

extern "C" {

// the workgroup's region in windows: a test picks a size whose window grid it does not divide
void emu_ssim_region(int *rw, int *rh) { *rw = SSIM_RW; *rh = SSIM_RH; }

// a = source, b = reconstruction: w x h luma, chroma 4:2:0, uint8 at 8 bit, uint16 at 10; order: SeqExec thread order (0 ascending, 1 descending, 2 random per
// phase); sum_q32, windows: three each.  Returns 0, or -3
int emu_ssim(const void *ay, const void *au, const void *av, const void *by, const void *bu, const void *bv, int w, int h, int bit_depth, int order,
             long long *sum_q32, long long *windows)
{
    if (w < 16 || h < 16 || (w & 7) || (h & 7) || (bit_depth != 8 && bit_depth != 10)) return -3;
    const void *a[3] = {ay, au, av}, *b[3] = {by, bu, bv};
    return bit_depth == 8 ? run<uint8_t>(a, b, w, h, order, sum_q32, windows) : run<uint16_t>(a, b, w, h, order, sum_q32, windows);
}

}  // extern "C"
