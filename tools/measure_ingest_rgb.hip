// tools/measure_ingest_rgb.hip — one k_ingest_rgb launch at 1920x1080 for the two sources DESIGN.md §6d names (rgb24 -> 8 bit, gbrp10le -> 10 bit) beside
// k_ingest on yuv444p -> 8 bit: device planes in, the session's plane layout out, 5 warm-up launches, then 30 timed ones, each between its own pair of HIP
// events; one JSON line per case.  Run it under `rocprofv3 --kernel-trace --stats` for the kernels' own device time (the event time includes the launch).
// A measurement tool, not part of the library; it launches the library's own kernels through csrc/device.h:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/measure_ingest_rgb.hip -Lhevc_amd -lmihevc -Wl,-rpath,'$ORIGIN/../hevc_amd' -o build/measure_ingest_rgb
#include <hip/hip_runtime.h>

#include <algorithm>
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

constexpr int W = 1920, H = 1080, PW = (W + 7) & ~7, PH = (H + 7) & ~7;

// n_planes source planes of row_elems x rows elements of es bytes; launch(src, dst, ostride) starts one conversion on stream 0
static int run(const char *name, int n_planes, int row_elems, size_t es, int out_depth,
               const std::function<hipError_t(void *const *, void *const *, const int *)> &launch)
{
    const size_t eo = out_depth > 8 ? 2 : 1;
    void *src[3] = {nullptr, nullptr, nullptr}, *dst[3];
    int ostride[3];
    size_t rd = 0, wr = 0;
    for (int c = 0; c < n_planes; c++) {
        CK(hipMalloc(&src[c], (size_t)row_elems * H * es));
        CK(hipMemset(src[c], 0x5A, (size_t)row_elems * H * es));
        rd += (size_t)row_elems * H * es;
    }
    for (int c = 0; c < 3; c++) {
        const int pwo = c ? PW / 2 : PW, pho = c ? PH / 2 : PH;
        ostride[c] = (pwo + 63) & ~63;
        CK(hipMalloc(&dst[c], (size_t)ostride[c] * pho * eo));
        wr += (size_t)pwo * pho * eo;
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> us;
    for (int i = 0; i < 35; i++) {
        CK(hipEventRecord(e0, 0));
        CK(launch(src, dst, ostride));
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (i >= 5) us.push_back(ms * 1000.0f);
    }
    std::sort(us.begin(), us.end());
    printf("{\"case\": \"%s -> 4:2:0 %d bit, 1920x1080\", \"launches\": %zu, \"median_us\": %.1f, \"min_us\": %.1f, \"max_us\": %.1f, \"bytes_read\": %zu, \"bytes_written\": %zu}\n",
           name, out_depth, us.size(), us[us.size() / 2], us.front(), us.back(), rd, wr);
    for (auto p : src) if (p) (void)hipFree(p);
    for (auto p : dst) (void)hipFree(p);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

static int run_rgb(const char *name, mihevc_rgb_format f, int out_depth)
{
    return run(name, rgb_planes(f), rgb_row_elems(f, W), (size_t)rgb_elem_size(f), out_depth, [&](void *const *src, void *const *dst, const int *ostride) {
        const IngestRgbArgs a = ingest_rgb_args(f, 1, false, src[0], src[1], src[2], rgb_row_elems(f, W), W, H, PW, PH, out_depth, dst, ostride);
        return launch_ingest_rgb(0, a, f.sample, rgb_elem_size(f), out_depth > 8);
    });
}

int main()
{
    const mihevc_src_format yuv444p = {444, 0, 8, 0, {0, 0, 0, 0}};
    if (run("yuv444p (k_ingest)", 3, W, 1, 8, [&](void *const *src, void *const *dst, const int *ostride) {
            const IngestArgs a = ingest_args(yuv444p, src[0], src[1], src[2], W, W, W, H, PW, PH, 8, dst, ostride);
            return launch_ingest(0, a, false, false);
        })) return 1;
    if (run_rgb("rgb24 (k_ingest_rgb)", mihevc_rgb_format{3, 0, 1, 2, 0, 8, 1, 1, {0, 0, 0, 0}}, 8)) return 1;
    return run_rgb("gbrp10le (k_ingest_rgb)", mihevc_rgb_format{0, 2, 0, 1, 0, 10, 1, 1, {0, 0, 0, 0}}, 10);
}
