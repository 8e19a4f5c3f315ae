// tools/measure_sr_compact.hip — HIP-event times of the compact super-resolution path.  1. The 64 -> 64 layer at 480x270 and 960x540:
// k_sr_compact against k_sr_conv<64, 4, false> (the RRDBNet path's kernel, with the LeakyReLU epilogue) on the same tensor and the same packed weights, in one
// binary, the two alternated over five rounds (per round and kernel 5 warm-up launches, then 30 timed ones, each between its own pair of events; median,
// fastest, slowest, and the achieved TFLOP/s).  2. Whole networks of 16 and 32 convolutions, x4, at both sizes (k_sr_input and every launch; 3 warm-up runs,
// 10 timed).  Gaussian weights and a random picture: zero operands would read high.  One JSON line per measurement.  `measure_sr_compact layer` runs only the
// 64 -> 64 k_sr_compact layer at 960x540: what a counter pass of its own is run over.  A measurement tool, not part of the library; it launches the library's own
// kernels through launch_sr_compact / launch_sr_conv / launch_sr_input / launch_sr_compact_network (csrc/device.h):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/measure_sr_compact.hip -Lhevc_amd -lmihevc -Wl,-rpath,'$ORIGIN/../hevc_amd' -o build/measure_sr_compact
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../hevc_amd/csrc/device.h"

using namespace mihevc;

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } \
    } while (0)

// median, fastest and slowest of `n` launches after `warm` warm-up ones, in microseconds
static int timed(const std::function<hipError_t()> &launch, int warm, int n, float (&us3)[3])
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> us;
    for (int i = 0; i < warm + n; i++) {
        CK(hipEventRecord(e0, 0));
        CK(launch());
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (i >= warm) us.push_back(ms * 1000.0f);
    }
    std::sort(us.begin(), us.end());
    us3[0] = us[us.size() / 2]; us3[1] = us.front(); us3[2] = us.back();
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

static int run(int convs, int sw, int sh, bool layer, bool both, bool whole)
{
    const size_t count = sr_compact_count(4, convs);
    std::vector<float> w(count);
    uint32_t rnd = 2463534242u;
    auto uni = [&]() { rnd ^= rnd << 13; rnd ^= rnd >> 17; rnd ^= rnd << 5; return (float)(rnd >> 8) / 16777216.0f; };
    for (auto &v : w) v = 0.04f * std::sqrt(-2.0f * std::log(uni() + 1e-7f)) * std::cos(6.2831853f * uni());
    SrCompactNet net;
    if (!sr_compact_build(4, convs, w.data(), count, net)) return 1;
    size_t off[SRC_BUFS];
    const size_t bytes = sr_compact_arena_layout(4, sw, sh, off);
    uint8_t *arena, *src;
    uint16_t *dw;
    float *dp;
    CK(hipMalloc(&arena, bytes));
    CK(hipMemset(arena, 0, bytes));
    CK(hipMalloc(&dw, net.wpk.size() * 2)); CK(hipMemcpy(dw, net.wpk.data(), net.wpk.size() * 2, hipMemcpyHostToDevice));
    CK(hipMalloc(&dp, net.par.size() * 4)); CK(hipMemcpy(dp, net.par.data(), net.par.size() * 4, hipMemcpyHostToDevice));
    std::vector<uint8_t> pic((size_t)3 * sw * sh);
    for (auto &b : pic) b = (uint8_t)(uni() * 256.0f);
    CK(hipMalloc(&src, pic.size())); CK(hipMemcpy(src, pic.data(), pic.size(), hipMemcpyHostToDevice));
    const mihevc_rgb_format fmt = {0, 0, 1, 2, 0, 8, 0, 0, {0, 0, 0, 0}};
    const void *planes[3] = {src, src + (size_t)sw * sh, src + (size_t)2 * sw * sh};
    const SrInputArgs ia = sr_input_args(fmt, 4, sw, sh, planes, sw, (uint16_t *)(arena + off[SRC_X]));
    // one whole frame first: every buffer then holds what the network leaves there
    CK(launch_sr_input(0, ia, 0, 1));
    CK(launch_sr_compact_network(0, net, arena, dw, dp, sw, sh));
    CK(hipDeviceSynchronize());
    float us[3];
    if (layer) {
        // trunk layer 0: A -> B
        const SrCompactLayer &y = net.layers[1];
        SrCompactArgs a;
        a.in = (const uint16_t *)(arena + off[SRC_A]); a.out = (uint16_t *)(arena + off[SRC_B]); a.wpk = dw + y.w_off; a.bias = dp + y.b_off; a.slope = dp + y.s_off;
        a.base = (const uint16_t *)(arena + off[SRC_X]); a.w = sw; a.h = sh;
        SrConvArgs c;
        c.in = a.in; c.out = a.out; c.wpk = a.wpk; c.bias = a.bias; c.r1 = c.r2 = a.in;
        c.in_ch = 64; c.in_off = 0; c.out_ch = 64; c.out_off = 0; c.r1_ch = c.r2_ch = 64; c.r1_off = c.r2_off = 0;
        c.w = sw; c.h = sh; c.up = 0; c.act = 1; c.n_res = 0; c.slope = 0.2f; c.a1 = c.a2 = 1.0f;
        const double flop = 2.0 * 9 * 64 * 64 * (double)sw * sh;
        for (int round = 0; round < (both ? 5 : 1); round++) {
            if (timed([&] { return launch_sr_compact(0, a, 64, 0); }, 5, 30, us)) return 1;
            printf("{\"case\": \"k_sr_compact 64 -> 64 at %dx%d\", \"round\": %d, \"median_us\": %.1f, \"min_us\": %.1f, \"max_us\": %.1f, \"tflops\": %.1f, \"workgroups\": %d}\n",
                   sw, sh, round, us[0], us[1], us[2], flop / us[0] * 1e-6, sr_compact_workgroups(sw, sh));
            if (!both) break;
            if (timed([&] { return launch_sr_conv(0, c, 64, 64, false); }, 5, 30, us)) return 1;
            printf("{\"case\": \"k_sr_conv 64 -> 64 at %dx%d\", \"round\": %d, \"median_us\": %.1f, \"min_us\": %.1f, \"max_us\": %.1f, \"tflops\": %.1f, \"workgroups\": %d}\n",
                   sw, sh, round, us[0], us[1], us[2], flop / us[0] * 1e-6, sr_conv_workgroups(sw, sh));
        }
    }
    if (whole) {
        if (timed([&] { hipError_t e = launch_sr_input(0, ia, 0, 1); return e != hipSuccess ? e : launch_sr_compact_network(0, net, arena, dw, dp, sw, sh); }, 3, 10, us)) return 1;
        double flop = 0;
        for (const SrCompactLayer &y : net.layers) flop += 2.0 * 9 * y.cin * y.cout * (double)sw * sh;
        printf("{\"case\": \"compact network x4 convs=%d %dx%d -> %dx%d\", \"median_ms\": %.3f, \"min_ms\": %.3f, \"max_ms\": %.3f, \"tflops\": %.1f, \"launches\": %zu, \"arena_mb\": %.0f}\n",
               convs, sw, sh, 4 * sw, 4 * sh, us[0] / 1000, us[1] / 1000, us[2] / 1000, flop / us[0] * 1e-6, net.launches.size() + 1, bytes / 1048576.0);
    }
    (void)hipFree(arena); (void)hipFree(dw); (void)hipFree(dp); (void)hipFree(src);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "layer")) return run(1, 960, 540, true, false, false);
    for (int size = 0; size < 2; size++) {
        const int sw = size ? 960 : 480, sh = size ? 540 : 270;
        if (run(1, sw, sh, true, true, false)) return 1;
        for (int convs : {16, 32})
            if (run(convs, sw, sh, false, false, true)) return 1;
    }
    return 0;
}
