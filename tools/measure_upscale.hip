// tools/measure_upscale.hip — HIP-event time of one k_upscale launch for the three cases DESIGN.md §6k names, each with the sharpener off and on, device planes
// in, the session's plane layout out, and beside each the time of k_scale at 1:1 onto the same output size (what merely writing those planes costs): 5 warm-up
// launches, then 30 timed ones, each between its own pair of events; one JSON line per measurement with the median, the fastest, the slowest and the bytes the
// definition moves (every source sample read once, every coded sample written once; the tables are a few tens of KB and stay in L2).  A measurement tool, not
// part of the library; it launches the library's own kernels through launch_upscale and launch_scale (csrc/device.h) over the tables of csrc/scale_taps.h:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/measure_upscale.hip -Lhevc_amd -lmihevc -Wl,-rpath,'$ORIGIN/../hevc_amd' -o build/measure_upscale
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <functional>
#include <vector>

#include "../hevc_amd/csrc/device.h"
#include "../hevc_amd/csrc/scale_taps.h"

using namespace mihevc;

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } \
    } while (0)

// median, fastest and slowest of 30 launches after 5 warm-up ones, in microseconds
static int timed(const std::function<hipError_t()> &launch, float (&us3)[3])
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> us;
    for (int i = 0; i < 35; i++) {
        CK(hipEventRecord(e0, 0));
        CK(launch());
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (i >= 5) us.push_back(ms * 1000.0f);
    }
    std::sort(us.begin(), us.end());
    us3[0] = us[us.size() / 2]; us3[1] = us.front(); us3[2] = us.back();
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

static int run(int sw, int sh, int dw, int dh, int bits)
{
    const int out_depth = bits, pw = (dw + 7) & ~7, ph = (dh + 7) & ~7;
    const size_t es = bits > 8 ? 2 : 1;
    UpscaleBlock blk;
    ScaleBlock one;
    if (!upscale_block_build(sw, sh, dw, dh, UP_TH, UP_HALO, UP_ROWS, blk) || !scale_block_build(dw, dh, dw, dh, SC_TH, SC_ROWS, one)) {
        fprintf(stderr, "no tables for %dx%d -> %dx%d\n", sw, sh, dw, dh);
        return 1;
    }
    // the source planes have the OUTPUT's size, so the 1:1 launch of k_scale reads them too; k_upscale reads their top left sw x sh samples at the same pitch
    void *src[3], *dst[3], *tab, *tab1;
    int ostride[3];
    size_t rd = 0, rd1 = 0, wr = 0;
    const int pitch_y = (dw + 15) & ~15, pitch_c = (dw / 2 + 15) & ~15;
    for (int c = 0; c < 3; c++) {
        const size_t bytes = (size_t)(c ? pitch_c : pitch_y) * (c ? dh / 2 : dh) * es;
        CK(hipMalloc(&src[c], bytes));
        CK(hipMemset(src[c], 0x5A, bytes));
        rd += (size_t)(c ? sw / 2 : sw) * (c ? sh / 2 : sh) * es;
        rd1 += (size_t)(c ? dw / 2 : dw) * (c ? dh / 2 : dh) * es;
    }
    for (int c = 0; c < 3; c++) {
        const int pwo = c ? pw / 2 : pw, pho = c ? ph / 2 : ph;
        ostride[c] = (pwo + 63) & ~63;
        CK(hipMalloc(&dst[c], (size_t)ostride[c] * pho * es));
        wr += (size_t)pwo * pho * es;
    }
    CK(hipMalloc(&tab, blk.bytes.size()));
    CK(hipMemcpy(tab, blk.bytes.data(), blk.bytes.size(), hipMemcpyHostToDevice));
    CK(hipMalloc(&tab1, one.bytes.size()));
    CK(hipMemcpy(tab1, one.bytes.data(), one.bytes.size(), hipMemcpyHostToDevice));
    const int32_t *first[4], *near[4], *first1[4];
    const int16_t *coef[4], *coef1[4];
    for (int k = 0; k < 4; k++) {
        first[k] = (const int32_t *)((uint8_t *)tab + blk.first[k]); near[k] = (const int32_t *)((uint8_t *)tab + blk.near[k]);
        coef[k] = (const int16_t *)((uint8_t *)tab + blk.coef[k]);
        first1[k] = (const int32_t *)((uint8_t *)tab1 + one.first[k]); coef1[k] = (const int16_t *)((uint8_t *)tab1 + one.coef[k]);
    }
    float us[3];
    const ScaleArgs a1 = scale_args(bits, src[0], src[1], src[2], pitch_y, pitch_c, dw, dh, dw, dh, pw, ph, out_depth, dst, ostride, first1, coef1, one.taps);
    if (timed([&] { return launch_scale(0, a1, es == 2, es == 2); }, us)) return 1;
    printf("{\"case\": \"k_scale %dx%d %d bit 1:1\", \"median_us\": %.1f, \"min_us\": %.1f, \"max_us\": %.1f, \"bytes_read\": %zu, \"bytes_written\": %zu, \"workgroups\": %d}\n",
           dw, dh, bits, us[0], us[1], us[2], rd1, wr, scale_workgroups(pw, ph));
    for (int g : {0, 8}) {
        const mihevc_upscale_src f = {sw, sh, bits, g, 8, {0, 0, 0}};
        const UpscaleArgs a = upscale_args(f, src[0], src[1], src[2], pitch_y, pitch_c, dw, dh, pw, ph, out_depth, dst, ostride, first, near, coef);
        if (timed([&] { return launch_upscale(0, a, es == 2, es == 2); }, us)) return 1;
        printf("{\"case\": \"k_upscale %dx%d -> %dx%d %d bit sharpen %d\", \"median_us\": %.1f, \"min_us\": %.1f, \"max_us\": %.1f, \"bytes_read\": %zu, \"bytes_written\": %zu, "
               "\"workgroups\": %d}\n", sw, sh, dw, dh, bits, g, us[0], us[1], us[2], rd, wr, upscale_workgroups(pw, ph));
    }
    for (auto p : src) (void)hipFree(p);
    for (auto p : dst) (void)hipFree(p);
    (void)hipFree(tab); (void)hipFree(tab1);
    return 0;
}

int main()
{
    if (run(960, 540, 1920, 1080, 8)) return 1;
    if (run(1280, 720, 1920, 1080, 8)) return 1;
    return run(1920, 1080, 3840, 2160, 10);
}
