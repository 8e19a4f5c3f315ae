// tools/measure_denoise.hip — HIP-event time of one k_denoise launch for the cases DESIGN.md §6g names, device planes in (three frames of pseudo-random
// samples, as a session's ring holds them), the session's plane layout out: 5 warm-up launches, then 30 timed ones, each between its own pair of events; one
// JSON line per case with the median, the fastest, the slowest and the bytes the definition moves (every sample of the three frames read once, every coded
// sample written once).  A measurement tool, not part of the library; it launches the library's own kernel through launch_denoise (csrc/device.h):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/measure_denoise.hip -Lhevc_amd -lmihevc -Wl,-rpath,'$ORIGIN/../hevc_amd' -o build/measure_denoise
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "../hevc_amd/csrc/device.h"

using namespace mihevc;

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } \
    } while (0)

static int run(int w, int h, int depth, const mihevc_denoise &dn)
{
    const int pw = (w + 7) & ~7, ph = (h + 7) & ~7;
    const size_t es = depth > 8 ? 2 : 1;
    void *src[3][3], *dst[3];
    int ostride[3];
    size_t rd = 0, wr = 0;
    const int pitch_y = (w + 15) & ~15, pitch_c = (w / 2 + 15) & ~15;
    uint32_t rnd = 2463534242u;
    for (int f = 0; f < 3; f++)
        for (int c = 0; c < 3; c++) {
            const size_t n = (size_t)(c ? pitch_c : pitch_y) * (c ? h / 2 : h);
            std::vector<uint8_t> host(n * es);
            for (size_t i = 0; i < n; i++) {
                rnd = rnd * 1664525u + 1013904223u;
                const unsigned v = (rnd >> 16) & ((1u << depth) - 1);
                if (es == 1) host[i] = (uint8_t)v; else { host[2 * i] = (uint8_t)v; host[2 * i + 1] = (uint8_t)(v >> 8); }
            }
            CK(hipMalloc(&src[f][c], n * es));
            CK(hipMemcpy(src[f][c], host.data(), n * es, hipMemcpyHostToDevice));
            rd += (size_t)(c ? w / 2 : w) * (c ? h / 2 : h) * es;
        }
    for (int c = 0; c < 3; c++) {
        const int pwo = c ? pw / 2 : pw, pho = c ? ph / 2 : ph;
        ostride[c] = (pwo + 63) & ~63;
        CK(hipMalloc(&dst[c], (size_t)ostride[c] * pho * es));
        wr += (size_t)pwo * pho * es;
    }
    const DenoiseArgs a = denoise_args(dn, depth, src[0], src[1], src[2], pitch_y, pitch_c, w, h, pw, ph, dst, ostride);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> us;
    for (int i = 0; i < 35; i++) {
        CK(hipEventRecord(e0, 0));
        CK(launch_denoise(0, a, es == 2));
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (i >= 5) us.push_back(ms * 1000.0f);
    }
    std::sort(us.begin(), us.end());
    printf("{\"case\": \"%dx%d %d bit strengths %d %d %d %d\", \"launches\": %zu, \"median_us\": %.1f, \"min_us\": %.1f, \"max_us\": %.1f, \"bytes_read\": %zu, \"bytes_written\": %zu, "
           "\"workgroups\": %d}\n",
           w, h, depth, dn.luma_spatial, dn.luma_temporal, dn.chroma_spatial, dn.chroma_temporal, us.size(), us[us.size() / 2], us.front(), us.back(), rd, wr, deint_workgroups(pw, ph));      // (the deinterlacer's tile and tile count serve k_denoise too)
    for (auto &f : src)
        for (auto p : f) (void)hipFree(p);
    for (auto p : dst) (void)hipFree(p);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

int main()
{
    const mihevc_denoise level2 = {5, 7, 5, 7, {0, 0, 0, 0}}, all = {255, 255, 255, 255, {0, 0, 0, 0}};
    if (run(1920, 1080, 8, level2)) return 1;
    if (run(1920, 1080, 8, all)) return 1;
    if (run(1920, 1080, 10, level2)) return 1;
    return run(3840, 2160, 10, level2);
}
