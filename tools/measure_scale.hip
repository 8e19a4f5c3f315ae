// tools/measure_scale.hip — HIP-event time of one k_scale launch for the three cases DESIGN.md §6e names, device planes in, the session's plane layout out:
// 5 warm-up launches, then 30 timed ones, each between its own pair of events; one JSON line per case with the median, the fastest, the slowest and the bytes
// the definition moves (every source sample read once, every coded sample written once; the tables are a few hundred KB and stay in L2).  A measurement tool,
// not part of the library; it launches the library's own kernel through launch_scale (csrc/device.h) over the tables of csrc/scale_taps.h:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/measure_scale.hip -Lhevc_amd -lmihevc -Wl,-rpath,'$ORIGIN/../hevc_amd' -o build/measure_scale
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "../hevc_amd/csrc/device.h"
#include "../hevc_amd/csrc/scale_taps.h"

using namespace mihevc;

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } \
    } while (0)

static int run(int sw, int sh, int dw, int dh, int bits, int out_depth)
{
    const int pw = (dw + 7) & ~7, ph = (dh + 7) & ~7;
    const size_t es = bits > 8 ? 2 : 1, eo = out_depth > 8 ? 2 : 1;
    ScaleBlock blk;
    if (!scale_block_build(sw, sh, dw, dh, SC_TH, SC_ROWS, blk)) { fprintf(stderr, "no tables for %dx%d -> %dx%d\n", sw, sh, dw, dh); return 1; }
    void *src[3], *dst[3], *tab;
    int ostride[3];
    size_t rd = 0, wr = 0;
    const int pitch_c = (sw / 2 + 15) & ~15;
    for (int c = 0; c < 3; c++) {
        const size_t bytes = (size_t)(c ? pitch_c : sw) * (c ? sh / 2 : sh) * es;
        CK(hipMalloc(&src[c], bytes));
        CK(hipMemset(src[c], 0x5A, bytes));
        rd += (size_t)(c ? sw / 2 : sw) * (c ? sh / 2 : sh) * es;
    }
    for (int c = 0; c < 3; c++) {
        const int pwo = c ? pw / 2 : pw, pho = c ? ph / 2 : ph;
        ostride[c] = (pwo + 63) & ~63;
        CK(hipMalloc(&dst[c], (size_t)ostride[c] * pho * eo));
        wr += (size_t)pwo * pho * eo;
    }
    CK(hipMalloc(&tab, blk.bytes.size()));
    CK(hipMemcpy(tab, blk.bytes.data(), blk.bytes.size(), hipMemcpyHostToDevice));
    const int32_t *first[4];
    const int16_t *coef[4];
    for (int k = 0; k < 4; k++) { first[k] = (const int32_t *)((uint8_t *)tab + blk.first[k]); coef[k] = (const int16_t *)((uint8_t *)tab + blk.coef[k]); }
    const ScaleArgs a = scale_args(bits, src[0], src[1], src[2], sw, pitch_c, sw, sh, dw, dh, pw, ph, out_depth, dst, ostride, first, coef, blk.taps);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> us;
    for (int i = 0; i < 35; i++) {
        CK(hipEventRecord(e0, 0));
        CK(launch_scale(0, a, es == 2, eo == 2));
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (i >= 5) us.push_back(ms * 1000.0f);
    }
    std::sort(us.begin(), us.end());
    printf("{\"case\": \"%dx%d %d bit -> %dx%d %d bit\", \"launches\": %zu, \"median_us\": %.1f, \"min_us\": %.1f, \"max_us\": %.1f, \"bytes_read\": %zu, \"bytes_written\": %zu, "
           "\"workgroups\": %d, \"taps\": [%d, %d, %d, %d]}\n",
           sw, sh, bits, dw, dh, out_depth, us.size(), us[us.size() / 2], us.front(), us.back(), rd, wr, scale_workgroups(pw, ph), blk.taps[0], blk.taps[1], blk.taps[2],
           blk.taps[3]);
    for (auto p : src) (void)hipFree(p);
    for (auto p : dst) (void)hipFree(p);
    (void)hipFree(tab);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

int main()
{
    if (run(3840, 2160, 1920, 1080, 8, 8)) return 1;
    if (run(3840, 2160, 1920, 1080, 10, 10)) return 1;
    return run(7680, 4320, 1920, 1080, 10, 10);
}
