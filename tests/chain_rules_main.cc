// tests/chain_rules_main.cc — hevc_amd/csrc/chain_plan.h restates, in a device-free header, the rules the entries of the single filters keep in their kernel
// headers (test_chain_cpu.py builds this stand-alone program): chain_check against the entries' OWN predicates over a grid of good and bad descriptors, so that
// the two statements cannot drift apart unnoticed.  Host code only.
#include <cstdio>
#include <memory>

#include "emu/ingest_planes.h"
#include "../hevc_amd/csrc/kernels/deint.h"
#include "../hevc_amd/csrc/kernels/denoise.h"
#include "../hevc_amd/csrc/kernels/fieldmatch.h"
#include "../hevc_amd/csrc/kernels/mcfi.h"
#include "../hevc_amd/csrc/kernels/scale.h"
#include "../hevc_amd/csrc/kernels/sr_yuv.h"
#include "../hevc_amd/csrc/kernels/upscale.h"
#include "../hevc_amd/csrc/sr_compact_net.h"
#include "../hevc_amd/csrc/sr_net.h"
#include "../hevc_amd/csrc/chain_plan.h"

using namespace mihevc;

// the chain's own rules (what no single entry states) and, per slot that is on, the predicates of that slot's entry
static bool entries_ok(const mihevc_chain &c, int W, int H, int D, int matrix, int sr_scale)
{
    auto side = [](int v) { return v >= 16 && v <= 8192 && !(v & 1); };
    auto depth = [](int d) { return d == 8 || d == 10; };
    if (!side(c.width) || !side(c.height) || !side(W) || !side(H) || !depth(c.bit_depth) || !depth(D)) return false;
    if (c.field < 0 || c.field > 2 || c.denoise_on < 0 || c.denoise_on > 1 || c.resize < 0 || c.resize > 3 || c.interpolate_on < 0 || c.interpolate_on > 1) return false;
    if (!c.field && !c.denoise_on && !c.resize && !c.interpolate_on) return false;
    for (int r : c.reserved)
        if (r) return false;
    const int sw = c.width, sh = c.height, sd = c.bit_depth;
    if (c.field && !(deint_geometry_ok(sw, sh) && (c.field == 1 ? deint_mode_ok(&c.deint) : fieldmatch_mode_ok(&c.fieldmatch)))) return false;
    if (c.denoise_on && !(denoise_geometry_ok(sw, sh) && denoise_strength_ok(&c.denoise))) return false;
    if (c.resize == 0 && (sw != W || sh != H || sd != D)) return false;
    if (c.resize == 1) {
        const mihevc_scale_src src = {sw, sh, sd, {0, 0, 0, 0, 0}};
        if (!scale_src_ok(&src) || !scale_geometry_ok(sw, sh, W, H)) return false;
    }
    if (c.resize == 2 && !(upscale_src_ok(&c.upscale) && c.upscale.width == sw && c.upscale.height == sh && c.upscale.bit_depth == sd && upscale_geometry_ok(sw, sh, W, H)))
        return false;
    if (c.resize == 3) {
        if (sr_scale != 2 && sr_scale != 4) return false;
        if (!sr_yuv_src_ok(&c.sr) || c.sr.width != sw || c.sr.height != sh || c.sr.bit_depth != sd || !rgb_matrix_ok(matrix)) return false;
        if (!sr_geometry_ok(sr_scale, sw, sh) || !sr_compact_geometry_ok(sw, sh)) return false;
        const int nw = sr_scale * sw, nh = sr_scale * sh;
        if (!(W == nw && H == nh) && !scale_geometry_ok(nw, nh, W, H)) return false;
    }
    if (c.interpolate_on && !(mcfi_geometry_ok(W, H) && mcfi_mode_ok(&c.interpolate))) return false;
    return true;
}

int main()
{
    long tried = 0, valid = 0, fails = 0;
    const int sizes[][2] = {{52, 36}, {100, 68}, {200, 136}, {400, 272}, {402, 272}, {400, 276}, {26, 18}, {24, 18}, {26, 16}, {100, 70}, {14, 68}, {101, 68}, {8192, 68}, {8194, 68}};
    const int sessions[][3] = {{100, 68, 8}, {100, 68, 10}, {104, 72, 8}, {208, 144, 8}, {100, 14, 8}, {99, 68, 8}, {100, 68, 12}};
    const int knobs[] = {-1, 0, 1, 2, 3, 4, 5, 8, 9, 64, 65, 255, 256};
    for (auto &sz : sizes)
        for (auto &ss : sessions)
            for (int depth : {8, 10, 12})
                for (int field = 0; field <= 2; field++)
                    for (int dn = 0; dn <= 1; dn++)
                        for (int resize = 0; resize <= 3; resize++)
                            for (int ip = 0; ip <= 1; ip++)
                                for (int knob : knobs)
                                    for (int where = 0; where < 12; where++)
                                        for (int sr_scale : {0, 2, 3, 4})
                                            for (int matrix : {1, 2}) {
                                                if ((sr_scale || matrix != 1) && resize != 3) continue;      // (they matter to the network's stage only)
                                                mihevc_chain c = {};
                                                c.width = sz[0]; c.height = sz[1]; c.bit_depth = depth;
                                                c.field = field; c.denoise_on = dn; c.resize = resize; c.interpolate_on = ip;
                                                c.deint.tff = 1; c.fieldmatch.tff = 1; c.fieldmatch.decimate = 1; c.fieldmatch.deint = 1;
                                                c.denoise.luma_spatial = c.denoise.chroma_spatial = 5; c.denoise.luma_temporal = c.denoise.chroma_temporal = 7;
                                                c.upscale.width = sz[0]; c.upscale.height = sz[1]; c.upscale.bit_depth = depth; c.upscale.sharpen = 8; c.upscale.antiring = 8;
                                                c.sr.width = sz[0]; c.sr.height = sz[1]; c.sr.bit_depth = depth; c.sr.matrix = 6;
                                                c.interpolate.factor = 2; c.interpolate.scene_threshold = 10;
                                                // one knob of one struct takes every value, in and out of its range
                                                int32_t *const at[12] = {&c.deint.field_rate, &c.deint.reserved[5], &c.fieldmatch.decimate, &c.fieldmatch.reserved[4], &c.denoise.chroma_temporal,
                                                                         &c.denoise.reserved[3], &c.upscale.sharpen, &c.upscale.antiring, &c.sr.matrix, &c.sr.full_range, &c.interpolate.factor,
                                                                         &c.interpolate.scene_threshold};
                                                *at[where] = knob;
                                                tried++;
                                                const bool got = chain_check(&c, ss[0], ss[1], ss[2], matrix, sr_scale), want = entries_ok(c, ss[0], ss[1], ss[2], matrix, sr_scale);
                                                valid += want;
                                                if (got != want && fails++ < 10)
                                                    std::printf("%dx%d@%d into %dx%d@%d field %d denoise %d resize %d interp %d knob %d = %d scale %d matrix %d: chain_check %d, the entries %d\n",
                                                                sz[0], sz[1], depth, ss[0], ss[1], ss[2], field, dn, resize, ip, where, knob, sr_scale, matrix, (int)got, (int)want);
                                            }
    if (fails) return 1;
    std::printf("%ld descriptors, %ld valid\n", tried, valid);
    return 0;
}
