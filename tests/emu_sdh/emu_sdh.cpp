// tests/emu_sdh/emu_sdh.cpp — TEST HARNESS, NOT PRODUCT.  tests/emu/emu.cpp stepped with sign data hiding switched on: the same sequential
// and four-wave executors over the same kernel sources, with CostParams::sign_hide taken from emu_set_sign_hide() instead of its default 0.
// emu.cpp builds its CostParams from the frozen 16-field mihevc_cost_params by aggregate initialisation; here that name is bound, for the text
// of emu.cpp only, to a type whose 16-argument constructor fills the same fields and then the switch.  Plus emu_transform_sdh, the stepped twin
// of mihevc_k_transform_sdh for 4x4 DCT and 8..32-point blocks (residual_pipeline on a pseudo-CTU), and emu_transform4_sdh, the stepped twin of its
// 4x4 path (k_transform4_blocks: transform4_program, DCT or DST-VII).  hevc_amd/ never loads this library.
#include "../../hevc_amd/csrc/kernels/common.h"
#include "../../hevc_amd/csrc/kernels/inter.h"
#include "../../hevc_amd/csrc/kernels/intra.h"
#include "../../hevc_amd/csrc/kernels/loopfilter.h"

static int g_sign_hide = 0;
struct SdhCostParams : mihevc::CostParams {
    SdhCostParams(int qp, int qp_c, int bd, int lsad, int lq4, int range, int tc, int tr, int nxn, int inp, int pre, int rz, int cm, int mt, int mb, int cg)
        : mihevc::CostParams{qp, qp_c, bd, lsad, lq4, range, tc, tr, nxn, inp, pre, rz, cm, mt, mb, cg}
    {
        sign_hide = g_sign_hide;
    }
};
#define CostParams SdhCostParams
#include "../emu/emu.cpp"
#undef CostParams

extern "C" {
void emu_set_sign_hide(int on) { g_sign_hide = on; }

// K3 on n_blocks blocks of 2^log2n (log2n 3..5: luma TUs of a pseudo-CTU, log2n 2: 4x4 DCT blocks in its chroma planes), every block in scan
// `scan`, with sign data hiding when sign_hide
int emu_transform_sdh(const int16_t *res, int16_t *lvl, int16_t *rec, int n_blocks, int log2n, int qp, int bit_depth, int intra, int scan, int sign_hide)
{
    if (log2n < 2 || log2n > 5 || scan < 0 || scan > 2) return -3;
    const int n = 1 << log2n, lt = log2n < 3 ? 3 : log2n, per = log2n == 2 ? 32 : 1024 >> (2 * log2n);       // blocks per pseudo-CTU
    // block b of a pseudo-CTU -> index of its top-left sample in the 1536-sample arrays
    auto origin = [&](int b) {
        if (log2n > 2) return (b / (32 >> log2n)) * n * 32 + (b % (32 >> log2n)) * n;
        return 1024 + (b >> 4) * 256 + ((b & 15) >> 2) * 4 * 16 + (b & 3) * 4;
    };
    SeqExec ex;
    for (int first = 0; first < n_blocks; first += per) {
        ResidualShared *s = fresh_shared<ResidualShared>();
        residual_init(ex, *s);
        ex.phase([&](int tid) {
            if (tid < 16) {
                const int blk = log2n > 2 ? first + ((tid >> 2) * 8 >> lt) * (32 >> lt) + ((tid & 3) * 8 >> lt) : first + tid;
                s->tu_log2[tid] = blk < n_blocks ? (uint8_t)lt : 0;
                s->tu_intra[tid] = (uint8_t)intra;
            }
            for (int i = tid; i < 1536; i += NT) s->res[i] = 0;
        });
        ex.phase([&](int tid) {
            for (int b = tid; b < per; b += NT) {
                if (first + b >= n_blocks) continue;
                const int o = origin(b), st = o < 1024 ? 32 : 16;
                for (int k = 0; k < n * n; k++) s->res[o + (k / n) * st + k % n] = res[(size_t)(first + b) * n * n + k];
            }
        });
        ex.phase([&](int tid) { for (int i = tid; i < 1536; i += NT) { SampleLoc l = locate(*s, i); l.scan = scan; s->desc[i] = pack_loc(l); } });
        residual_pipeline(ex, *s, qp, qp, bit_depth, whole_ctu(), 0, sign_hide);
        for (int b = 0; b < per && first + b < n_blocks; b++) {
            const int o = origin(b), st = o < 1024 ? 32 : 16;
            for (int k = 0; k < n * n; k++) {
                lvl[(size_t)(first + b) * n * n + k] = s->lvl[o + (k / n) * st + k % n];
                rec[(size_t)(first + b) * n * n + k] = s->res[o + (k / n) * st + k % n];
            }
        }
        free(s);
    }
    return 0;
}

// k_transform4_blocks on n_blocks 4x4 blocks (DST-VII when dst, else DCT), the same grid of NT / 16 blocks per workgroup
int emu_transform4_sdh(const int16_t *res, int16_t *lvl, int16_t *rec, int n_blocks, int qp, int bit_depth, int intra, int dst, int scan, int sign_hide)
{
    if (scan < 0 || scan > 2) return -3;
    SeqExec ex;
    for (int first = 0; first < n_blocks; first += NT / 16) {
        Transform4Shared *s = fresh_shared<Transform4Shared>();
        transform4_program(ex, *s, res, lvl, rec, n_blocks, first, qp, bit_depth, intra, dst, scan, sign_hide);
        free(s);
    }
    return 0;
}
}
