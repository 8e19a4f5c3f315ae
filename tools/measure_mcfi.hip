// tools/measure_mcfi.hip — HIP-event times of k_mcfi_search, k_mcfi_field and k_mcfi_render for the cases DESIGN.md §6j names, device planes in (two frames of a
// smooth synthetic texture, the second moved by (10, -6) samples, as a session's ring holds them), the session's plane layout out: 5 warm-up launches, then 30
// timed ones, each between its own pair of events; one JSON line per case and kernel with the median, the fastest and the slowest.  The render is timed at
// picture 1 of 2 with the field the two other kernels left, no scene check.  A measurement tool, not part of the library; it launches the library's own kernels
// through launch_mcfi_search, launch_mcfi_field and launch_mcfi_render (csrc/device.h):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/measure_mcfi.hip -Lhevc_amd -lmihevc -Wl,-rpath,'$ORIGIN/../hevc_amd' -o build/measure_mcfi
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <functional>
#include <vector>

#include "../hevc_amd/csrc/device.h"

using namespace mihevc;

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } \
    } while (0)

static int timed(const char *what, int w, int h, int depth, int workgroups, const std::function<hipError_t()> &launch)
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
    printf("{\"case\": \"%dx%d %d bit\", \"kernel\": \"%s\", \"launches\": %zu, \"median_us\": %.1f, \"min_us\": %.1f, \"max_us\": %.1f, \"workgroups\": %d}\n", w, h, depth, what,
           us.size(), us[us.size() / 2], us.front(), us.back(), workgroups);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

static int run(int w, int h, int depth)
{
    const int pw = (w + 7) & ~7, ph = (h + 7) & ~7;
    const size_t es = depth > 8 ? 2 : 1;
    void *src[2][3], *dst[3], *blk;
    int ostride[3];
    const int pitch_y = (w + 15) & ~15, pitch_c = (w / 2 + 15) & ~15;
    for (int f = 0; f < 2; f++)
        for (int c = 0; c < 3; c++) {
            const int pitch = c ? pitch_c : pitch_y, rows = c ? h / 2 : h, sc = c ? 2 : 1;
            const size_t n = (size_t)pitch * rows;
            std::vector<uint8_t> host(n * es);
            for (int y = 0; y < rows; y++)
                for (int x = 0; x < pitch; x++) {
                    const double X = sc * x - 10.0 * f, Y = sc * y + 6.0 * f;
                    const double t = 0.5 + 0.22 * std::sin(0.07 * X + 0.031 * Y) + 0.15 * std::sin(0.013 * X - 0.09 * Y) + 0.08 * std::sin(0.61 * X + 0.47 * Y);
                    const unsigned v = (unsigned)(t * ((1u << depth) - 1));
                    const size_t i = (size_t)y * pitch + x;
                    if (es == 1) host[i] = (uint8_t)v; else { host[2 * i] = (uint8_t)v; host[2 * i + 1] = (uint8_t)(v >> 8); }
                }
            CK(hipMalloc(&src[f][c], n * es));
            CK(hipMemcpy(src[f][c], host.data(), n * es, hipMemcpyHostToDevice));
        }
    for (int c = 0; c < 3; c++) {
        const int pwo = c ? pw / 2 : pw, pho = c ? ph / 2 : ph;
        ostride[c] = (pwo + 63) & ~63;
        CK(hipMalloc(&dst[c], (size_t)ostride[c] * pho * es));
    }
    const McfiLayout l = mcfi_layout(w, h);
    CK(hipMalloc(&blk, l.bytes));
    const McfiSearchArgs sa = mcfi_search_args(depth, src[0][0], src[1][0], pitch_y, w, h, (uint8_t *)blk);
    const McfiFieldArgs fa = mcfi_field_args(sa, (uint8_t *)blk);
    const mihevc_interpolate m = {2, 0, 0, {0, 0, 0, 0, 0}};
    const McfiRenderArgs ra = mcfi_render_args(m, 1, depth, src[0], src[1], pitch_y, pitch_c, w, h, pw, ph, fa.v, fa.dsum, dst, ostride);
    if (timed("k_mcfi_search", w, h, depth, mcfi_search_workgroups(w, h), [&] { return launch_mcfi_search(0, sa, es == 2); })) return 1;
    if (timed("k_mcfi_field", w, h, depth, mcfi_field_workgroups(w, h), [&] { return launch_mcfi_field(0, fa, es == 2); })) return 1;
    if (timed("k_mcfi_render", w, h, depth, mcfi_render_workgroups(pw, ph), [&] { return launch_mcfi_render(0, ra, es == 2); })) return 1;
    std::vector<int16_t> v((size_t)sa.nbx * sa.nby * 2);
    CK(hipMemcpy(v.data(), fa.v, v.size() * 2, hipMemcpyDeviceToHost));
    size_t moving = 0;
    for (size_t b = 0; b < v.size() / 2; b++) moving += v[2 * b] == 5 && v[2 * b + 1] == -3;
    printf("{\"case\": \"%dx%d %d bit\", \"blocks\": %zu, \"blocks_with_the_true_vector\": %zu}\n", w, h, depth, v.size() / 2, moving);
    for (auto &f : src)
        for (auto p : f) (void)hipFree(p);
    for (auto p : dst) (void)hipFree(p);
    (void)hipFree(blk);
    return 0;
}

int main()
{
    if (run(1920, 1080, 8)) return 1;
    return run(3840, 2160, 10);
}
