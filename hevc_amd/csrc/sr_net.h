// hevc_amd/csrc/sr_net.h — an RRDBNet as kernels/sr_conv.h runs it: the weights packed into MFMA fragments, the list of launches and the
// device memory a source size needs.  Host arithmetic only, no HIP: the session, the stage entries and the tests (tests/emu/sr.cpp) share it.
// Network: num_feat 64, num_grow_ch 32, `blocks` >= 1 RRDBs, scale 4 or 2 (scale 2 starts with a pixel-unshuffle: 12 input channels).  SRVGGNetCompact (realesr-general with its
// denoise blend) is sr_compact_net.h.  Out of scope: other architectures, scale 1, other channel counts, tiling, frames too large for memory, fp8 / int8.
//   flat weights   fp32, layer after layer, each layer its weight in torch's order [cout][cin][3][3], then its bias [cout]:
//                  conv_first (cin 3 or 12), then for block i = 0 .., rdb 1 .. 3, conv 1 .. 5 (cin 64 + 32 (k - 1), cout 32, conv5: 64), then conv_body,
//                  conv_up1, conv_up2, conv_hr (64 -> 64) and conv_last (64 -> 3)
//   packed weights halves (fp32 rounded to nearest even); per layer [step = tap * cin_pad / 32 + chunk][fragment n of 16 output channels][lane 0 .. 63][8]:
//                  element j of lane l is W[co = 16 n + (l & 15)][ci = 32 chunk + 8 (l >> 4) + j][ky = tap / 3][kx = tap % 3], zero where co or ci is padding
//                  (cin 3 / 12 -> 32, cout 3 -> 16).  Biases stay fp32, zero padded to 16 n
//   buffers        T = tw x th pixels of the input tensor (the source, or half of it each way at scale 2):
//                  X 32 ch; FEA 64; D0, D1, D2 192 each (a dense block's concatenation: its input in channels 0 .. 63, x1 .. x4 behind); U1 64 ch of 4 T pixels;
//                  U2, U3 64 ch of 16 T; OUT three planes of 16 T.  One arena, every buffer at a multiple of 256 bytes:
//                  bytes = sum of the above x 2, about 6048 T (sr_net_bytes states it exactly).  Nothing is tiled: a size whose arena cannot be allocated is
//                  MIHEVC_ENOMEM
//   launches       conv_first runs twice, into FEA (kept for the trunk's sum) and into D0[0:64] (the first block's input): one launch has one output, and the
//                  layer is 1/300 of the network.  An RRDB finds its input in D0[0:64]; RDB1 works in D0 and leaves its result in D1[0:64], RDB2 D1 -> D2,
//                  RDB3 in D2 writes (v 0.2 + D2[0:64]) 0.2 + D0[0:64] over D0[0:64]: a lane reads the residual of exactly the elements it then stores
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "kernels/sr_conv.h"

namespace mihevc {

enum { SR_X, SR_FEA, SR_D0, SR_D1, SR_D2, SR_U1, SR_U2, SR_U3, SR_OUT, SR_BUFS };
inline int sr_buf_channels(int b) { return b == SR_X ? SR_CIN0 : b == SR_D0 || b == SR_D1 || b == SR_D2 ? 192 : b == SR_OUT ? 3 : 64; }
inline int sr_buf_level(int b) { return b == SR_U1 ? 1 : b == SR_U2 || b == SR_U3 || b == SR_OUT ? 2 : 0; }      // pixels = T << 2 level

struct SrLayer {
    int cin, cout, cin_pad, cout_pad;
    size_t w_off, b_off;            // into SrNet::wpk (halves) and SrNet::bias
};
struct SrLaunch {
    int layer;
    int in_buf, in_off, out_buf, out_off;
    int level;                      // of the output
    int up, planar, act, n_res;
    float a1, a2;
    int r1_buf, r1_off, r2_buf, r2_off;
};
struct SrNet {
    int scale = 0, blocks = 0;
    std::vector<uint16_t> wpk;
    std::vector<float> bias;
    std::vector<SrLayer> layers;
    std::vector<SrLaunch> launches;
};

inline bool sr_model_ok(const mihevc_sr_model *m)
{
    if (!m || (m->scale != 2 && m->scale != 4) || m->blocks < 1 || m->blocks > 64) return false;
    for (int i = 0; i < 6; i++)
        if (m->reserved[i]) return false;
    return true;
}
// the source sizes a network takes: at least 4 each way, even at scale 2, and an output the session limits allow
inline bool sr_geometry_ok(int scale, int sw, int sh)
{
    return sw >= 4 && sh >= 4 && sw <= 8192 && sh <= 8192 && (scale == 4 || !((sw | sh) & 1));
}
inline void sr_layer_shapes(int scale, int blocks, std::vector<SrLayer> &l)
{
    auto add = [&](int cin, int cout) { l.push_back(SrLayer{cin, cout, (cin + SR_K - 1) / SR_K * SR_K, (cout + SR_M - 1) / SR_M * SR_M, 0, 0}); };
    l.clear();
    add(scale == 2 ? 12 : 3, 64);
    for (int i = 0; i < blocks * 3; i++)
        for (int k = 0; k < 5; k++) add(64 + 32 * k, k == 4 ? 64 : 32);
    for (int k = 0; k < 4; k++) add(64, 64);
    add(64, 3);
}
// number of floats of the flat weights
inline size_t sr_net_count(int scale, int blocks)
{
    std::vector<SrLayer> l;
    sr_layer_shapes(scale, blocks, l);
    size_t n = 0;
    for (const SrLayer &y : l) n += (size_t)y.cout * y.cin * 9 + y.cout;
    return n;
}
// one layer's fp32 weights [cout][cin][3][3] -> 9 * cin_pad / 32 * cout_pad / 16 * 64 * 8 halves
inline void sr_pack_layer(const float *w, int cout, int cin, int cout_pad, int cin_pad, uint16_t *dst)
{
    const int kc_n = cin_pad / SR_K, nb = cout_pad / SR_M;
    for (int tap = 0; tap < 9; tap++)
        for (int kc = 0; kc < kc_n; kc++)
            for (int n = 0; n < nb; n++)
                for (int l = 0; l < 64; l++)
                    for (int j = 0; j < 8; j++) {
                        const int co = SR_M * n + (l & 15), ci = SR_K * kc + 8 * (l >> 4) + j;
                        const float v = co < cout && ci < cin ? w[((size_t)co * cin + ci) * 9 + tap] : 0.0f;
                        dst[((((size_t)tap * kc_n + kc) * nb + n) * 64 + l) * 8 + j] = sr_half_of_float_sw(v);
                    }
}
inline size_t sr_packed_halves(int cout_pad, int cin_pad) { return (size_t)9 * cin_pad * cout_pad; }

inline bool sr_net_build(int scale, int blocks, const float *weights, size_t count, SrNet &net)
{
    if ((scale != 2 && scale != 4) || blocks < 1 || !weights || count != sr_net_count(scale, blocks)) return false;
    net.scale = scale; net.blocks = blocks;
    sr_layer_shapes(scale, blocks, net.layers);
    size_t wn = 0, bn = 0;
    for (SrLayer &y : net.layers) { y.w_off = wn; y.b_off = bn; wn += sr_packed_halves(y.cout_pad, y.cin_pad); bn += (size_t)y.cout_pad; }
    net.wpk.assign(wn, 0);
    net.bias.assign(bn, 0.0f);
    const float *p = weights;
    for (const SrLayer &y : net.layers) {
        sr_pack_layer(p, y.cout, y.cin, y.cout_pad, y.cin_pad, net.wpk.data() + y.w_off);
        p += (size_t)y.cout * y.cin * 9;
        for (int c = 0; c < y.cout; c++) net.bias[y.b_off + c] = p[c];
        p += y.cout;
    }
    net.launches.clear();
    auto conv = [&](int layer, int in_buf, int out_buf, int out_off, int act) {
        net.launches.push_back(SrLaunch{layer, in_buf, 0, out_buf, out_off, sr_buf_level(out_buf), 0, 0, act, 0, 1.0f, 1.0f, 0, 0, 0, 0});
        return &net.launches.back();
    };
    int layer = 0;
    conv(layer, SR_X, SR_FEA, 0, 0);
    conv(layer++, SR_X, SR_D0, 0, 0);
    const int dense[3] = {SR_D0, SR_D1, SR_D2};
    for (int b = 0; b < blocks; b++)
        for (int r = 0; r < 3; r++) {
            for (int k = 0; k < 4; k++) conv(layer++, dense[r], dense[r], 64 + 32 * k, 1);
            SrLaunch *c5 = conv(layer++, dense[r], r == 2 ? SR_D0 : dense[r + 1], 0, 0);
            c5->n_res = r == 2 ? 2 : 1; c5->a1 = 0.2f; c5->r1_buf = dense[r];
            if (r == 2) { c5->a2 = 0.2f; c5->r2_buf = SR_D0; }
        }
    SrLaunch *body = conv(layer++, SR_D0, SR_FEA, 0, 0);
    body->n_res = 1; body->a1 = 1.0f; body->r1_buf = SR_FEA;
    conv(layer++, SR_FEA, SR_U1, 0, 1)->up = 1;
    conv(layer++, SR_U1, SR_U2, 0, 1)->up = 1;
    conv(layer++, SR_U2, SR_U3, 0, 1);
    conv(layer++, SR_U3, SR_OUT, 0, 0)->planar = 1;
    return layer == (int)net.layers.size();
}

// k_sr_input's arguments from a format: the source planes at p, the tensor at out
inline SrInputArgs sr_input_args(const mihevc_rgb_format &f, int scale, int sw, int sh, const void *const *p, int pitch, uint16_t *out)
{
    SrInputArgs a;
    for (int c = 0; c < 3; c++) a.src[c] = c < rgb_planes(f) ? p[c] : nullptr;
    a.out = out; a.pitch = pitch; a.epp = f.layout ? f.layout : 1;
    a.pos[0] = f.r; a.pos[1] = f.g; a.pos[2] = f.b;
    a.vmax = f.sample ? 65535 : (1 << f.bit_depth) - 1;
    a.sw = sw; a.sh = sh; a.unshuffle = scale == 2;
    return a;
}
// the arena: offset of every buffer and the total, in bytes, for an input tensor of tw x th pixels
inline size_t sr_arena_layout(int tw, int th, size_t (&off)[SR_BUFS])
{
    size_t n = 0;
    for (int b = 0; b < SR_BUFS; b++) {
        off[b] = n;
        n += (((size_t)tw * th << (2 * sr_buf_level(b))) * sr_buf_channels(b) * 2 + 255) & ~(size_t)255;
    }
    return n;
}
// device bytes a source of sw x sh needs: the arena, the staged source aside
inline size_t sr_net_bytes(int scale, int sw, int sh)
{
    size_t off[SR_BUFS];
    const int f = scale == 2 ? 2 : 1;
    return sr_arena_layout(sw / f, sh / f, off);
}
// the kernel arguments of launch `l` over an arena at `arena` with packed weights at `wpk` / `bias` (device or host addresses alike)
inline SrConvArgs sr_launch_args(const SrNet &net, const SrLaunch &l, uint8_t *arena, const uint16_t *wpk, const float *bias, int tw, int th, float slope)
{
    size_t off[SR_BUFS];
    sr_arena_layout(tw, th, off);
    const SrLayer &y = net.layers[(size_t)l.layer];
    SrConvArgs a;
    a.in = (const uint16_t *)(arena + off[l.in_buf]); a.out = (uint16_t *)(arena + off[l.out_buf]);
    a.wpk = wpk + y.w_off; a.bias = bias + y.b_off;
    a.r1 = (const uint16_t *)(arena + off[l.r1_buf]); a.r2 = (const uint16_t *)(arena + off[l.r2_buf]);
    a.in_ch = sr_buf_channels(l.in_buf); a.in_off = l.in_off; a.out_ch = sr_buf_channels(l.out_buf); a.out_off = l.out_off;
    a.r1_ch = sr_buf_channels(l.r1_buf); a.r1_off = l.r1_off; a.r2_ch = sr_buf_channels(l.r2_buf); a.r2_off = l.r2_off;
    a.w = tw << l.level; a.h = th << l.level;
    a.up = l.up; a.act = l.act; a.n_res = l.n_res; a.slope = slope; a.a1 = l.a1; a.a2 = l.a2;
    return a;
}
// Runs `fn(cin_pad, cout_pad, planar, args)` for every launch of the network in order: the one place that walks the list
template <class F> inline int sr_for_each_launch(const SrNet &net, uint8_t *arena, const uint16_t *wpk, const float *bias, int tw, int th, F &&fn)
{
    for (const SrLaunch &l : net.launches) {
        const SrLayer &y = net.layers[(size_t)l.layer];
        if (int e = fn(y.cin_pad, y.cout_pad, l.planar != 0, sr_launch_args(net, l, arena, wpk, bias, tw, th, 0.2f))) return e;
    }
    return 0;
}

}  // namespace mihevc
