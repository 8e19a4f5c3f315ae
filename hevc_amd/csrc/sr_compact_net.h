// hevc_amd/csrc/sr_compact_net.h — a compact super-resolution network (SRVGGNetCompact) as kernels/sr_compact.h runs it: the weights packed
// into MFMA fragments, the list of launches and the device memory a source size needs.  Host arithmetic only, no HIP: the session, the stage entries and the
// tests (tests/emu/sr_compact.cpp) share it.  The sibling of sr_net.h (RRDBNet), whose packer (sr_pack_layer) it uses.
// Network: num_feat 64, `convs` trunk layers (16 in realesr-animevideov3, 32 in realesr-general-x4v3 and -wdn-x4v3), scale r = 4 or 2:
//   conv(3 -> 64) PReLU; convs x (conv(64 -> 64) PReLU); conv(64 -> 3 r r); PixelShuffle(r); + the source enlarged r times by nearest.
// There is no pixel-unshuffle at scale 2: the input tensor is the source at its own size at either scale, so odd source sides are fine.
//   flat weights   fp32, torch's state-dict order: body.0.weight [64][3][3][3], body.0.bias [64], body.1.weight [64] (the PReLU slopes); then per trunk layer
//                  weight [64][64][3][3], bias [64], slopes [64]; then the last convolution's weight [3 r r][64][3][3] and bias [3 r r].
//                  sr_compact_count gives the number of floats
//   packed weights sr_pack_layer's fragment order (sr_net.h), cin 3 -> 32, cout 12 -> 16; biases and slopes stay fp32, in one array `par`: per layer the
//                  biases (zero padded to the fragments), then for every layer but the last its 64 slopes
//   buffers        T = sw x sh source pixels: X 32 channels (k_sr_input / k_sr_from_yuv, as for an RRDBNet of scale 4), A and B 64 channels, OUT three planes of
//                  r r T.  One arena, every buffer at a multiple of 256 bytes: 64 + 128 + 128 + 6 r r bytes a source pixel, 416 at r = 4
//                  (sr_compact_bytes states the total exactly).  Nothing is tiled: a size whose arena cannot be allocated is MIHEVC_ENOMEM
//   launches       convs + 2 of k_sr_compact: the first layer X -> A, trunk layer i (0 ..) from A to B when i is even and from B to A when odd, the tail
//                  from where the trunk ended -> OUT, with X as its base
// Out of scope: scale 3 and 1, num_feat other than 64, fusing layers, fp8 / int8, tiling, batching.
#pragma once
#include "sr_net.h"
#include "kernels/sr_compact.h"

namespace mihevc {

enum { SRC_X, SRC_A, SRC_B, SRC_OUT, SRC_BUFS };

struct SrCompactLayer {
    int cin, cout, cin_pad, cout_pad;
    size_t w_off, b_off, s_off;      // into SrCompactNet::wpk (halves) and ::par (floats); s_off: the slopes (the last layer has none)
};
struct SrCompactLaunch {
    int layer, in_buf, out_buf, tail;      // tail: 0, or the scale
};
struct SrCompactNet {
    int scale = 0, convs = 0;
    std::vector<uint16_t> wpk;
    std::vector<float> par;
    std::vector<SrCompactLayer> layers;
    std::vector<SrCompactLaunch> launches;
};

inline bool sr_compact_ok(const mihevc_sr_compact *m)
{
    if (!m || (m->scale != 2 && m->scale != 4) || m->convs < 1 || m->convs > 64) return false;
    for (int i = 0; i < 6; i++)
        if (m->reserved[i]) return false;
    return true;
}
// the source sizes a compact network takes: at least 4 each way and an output the session limits allow
inline bool sr_compact_geometry_ok(int sw, int sh) { return sw >= 4 && sh >= 4 && sw <= 8192 && sh <= 8192; }
// number of floats of the flat weights
inline size_t sr_compact_count(int scale, int convs)
{
    const size_t last = (size_t)3 * scale * scale;
    return (size_t)(64 * 3 * 9 + 128) + (size_t)convs * (64 * 64 * 9 + 128) + last * 64 * 9 + last;
}
inline int sr_compact_launches(int convs) { return convs + 2; }

inline bool sr_compact_build(int scale, int convs, const float *weights, size_t count, SrCompactNet &net)
{
    if ((scale != 2 && scale != 4) || convs < 1 || !weights || count != sr_compact_count(scale, convs)) return false;
    net.scale = scale; net.convs = convs;
    net.layers.clear();
    auto add = [&](int cin, int cout) { net.layers.push_back(SrCompactLayer{cin, cout, (cin + SR_K - 1) / SR_K * SR_K, (cout + SR_M - 1) / SR_M * SR_M, 0, 0, 0}); };
    add(3, 64);
    for (int i = 0; i < convs; i++) add(64, 64);
    add(64, 3 * scale * scale);
    size_t wn = 0, pn = 0;
    for (size_t i = 0; i < net.layers.size(); i++) {
        SrCompactLayer &y = net.layers[i];
        y.w_off = wn; y.b_off = pn;
        wn += sr_packed_halves(y.cout_pad, y.cin_pad); pn += (size_t)y.cout_pad;
        y.s_off = pn;
        if (i + 1 < net.layers.size()) pn += 64;
    }
    net.wpk.assign(wn, 0);
    net.par.assign(pn, 0.0f);
    const float *p = weights;
    for (size_t i = 0; i < net.layers.size(); i++) {
        const SrCompactLayer &y = net.layers[i];
        sr_pack_layer(p, y.cout, y.cin, y.cout_pad, y.cin_pad, net.wpk.data() + y.w_off);
        p += (size_t)y.cout * y.cin * 9;
        for (int c = 0; c < y.cout; c++) net.par[y.b_off + c] = p[c];
        p += y.cout;
        if (i + 1 < net.layers.size()) {
            for (int c = 0; c < 64; c++) net.par[y.s_off + c] = p[c];
            p += 64;
        }
    }
    net.launches.clear();
    net.launches.push_back(SrCompactLaunch{0, SRC_X, SRC_A, 0});
    int cur = SRC_A;
    for (int i = 0; i < convs; i++) {
        const int nxt = cur == SRC_A ? SRC_B : SRC_A;
        net.launches.push_back(SrCompactLaunch{1 + i, cur, nxt, 0});
        cur = nxt;
    }
    net.launches.push_back(SrCompactLaunch{1 + convs, cur, SRC_OUT, scale});
    return p == weights + count;
}

// the arena: offset of every buffer and the total, in bytes, for a source of sw x sh pixels
inline size_t sr_compact_arena_layout(int scale, int sw, int sh, size_t (&off)[SRC_BUFS])
{
    const size_t px = (size_t)sw * sh, per[SRC_BUFS] = {SR_CIN0 * 2, 128, 128, (size_t)6 * scale * scale};
    size_t n = 0;
    for (int b = 0; b < SRC_BUFS; b++) {
        off[b] = n;
        n += (px * per[b] + 255) & ~(size_t)255;
    }
    return n;
}
// device bytes a source of sw x sh needs: the arena, the staged source aside
inline size_t sr_compact_bytes(int scale, int sw, int sh)
{
    size_t off[SRC_BUFS];
    return sr_compact_arena_layout(scale, sw, sh, off);
}
// Runs `fn(cin_pad, tail, args)` for every launch of the network in order over an arena at `arena` with the packed weights at `wpk` and the biases and slopes
// at `par` (device or host addresses alike): the one place that walks the list
template <class F> inline int sr_compact_for_each_launch(const SrCompactNet &net, uint8_t *arena, const uint16_t *wpk, const float *par, int sw, int sh, F &&fn)
{
    size_t off[SRC_BUFS];
    sr_compact_arena_layout(net.scale, sw, sh, off);
    for (const SrCompactLaunch &l : net.launches) {
        const SrCompactLayer &y = net.layers[(size_t)l.layer];
        SrCompactArgs a;
        a.in = (const uint16_t *)(arena + off[l.in_buf]); a.out = (uint16_t *)(arena + off[l.out_buf]);
        a.wpk = wpk + y.w_off; a.bias = par + y.b_off; a.slope = par + y.s_off;
        a.base = (const uint16_t *)(arena + off[SRC_X]);
        a.w = sw; a.h = sh;
        if (int e = fn(y.cin_pad, l.tail, a)) return e;
    }
    return 0;
}

}  // namespace mihevc
