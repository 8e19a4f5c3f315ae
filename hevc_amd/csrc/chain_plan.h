// hevc_amd/csrc/chain_plan.h — the rules of a source filter chain (mihevc_set_source_chain): which descriptors are valid, the size and depth every
// stage runs at, the rate the chain multiplies the source's by and the pictures n frames give.  Pure arithmetic over the descriptor (no HIP;
// tests/chain_asan_main.cc runs it alone), restated here from the entries of the single filters so that the entry, mihevc_chain_plan_for and through it Python
// read one set of rules; tests/chain_rules_main.cc holds chain_check against the entries' own predicates (the kernel headers', which a device-free header cannot
// include), so the restatement cannot drift.
//   order      field (deint | fieldmatch) -> denoise -> resize (scale | upscale | sr) -> interpolate; every slot optional, at least one on
//   sizes      field and denoise run at the source's size and depth, resize takes the source to the session, interpolate runs at the session's size and depth
//   rate       field rate x2, decimate x4/5, interpolate x factor, as one reduced fraction
//   pictures   n frames: 2n at field rate, n - n / 5 when decimating (a partial last cycle comes out whole), then factor (m - 1) + 1 behind the interpolator
#pragma once
#include <cstdint>

#include "../../include/mihevc.h"

namespace mihevc {

struct ChainPlan {
    bool field, denoise, resize, interp;      // the slots that are on
    int sw, sh, sd;                           // what the field and denoise stages run at: the source
    int dw, dh, dd;                           // what the resize stage writes and the interpolator runs at: the session
    int rate_num, rate_den;                   // pictures per source frame in the long run, reduced
    int stages;                               // slots that are on
};

inline bool chain_flag_ok(int v) { return v == 0 || v == 1; }
inline bool chain_zero(const int32_t *r, int n)
{
    int32_t acc = 0;
    for (int i = 0; i < n; i++) acc |= r[i];
    return acc == 0;
}
inline bool chain_matrix_ok(int m) { return m == 1 || m == 5 || m == 6 || m == 9; }
inline bool chain_side_ok(int v) { return v >= 16 && v <= 8192 && !(v & 1); }

// The descriptor against a session of W x H at `depth` whose colour matrix is `matrix`; sr_scale: the scale of the session's network, 0 without one.  The
// embedded structs of slots that are off are not looked at
inline bool chain_check(const mihevc_chain *c, int W, int H, int depth, int matrix, int sr_scale)
{
    if (!c || !chain_zero(c->reserved, 9)) return false;
    if (!chain_side_ok(c->width) || !chain_side_ok(c->height) || (c->bit_depth != 8 && c->bit_depth != 10)) return false;
    if (!chain_side_ok(W) || !chain_side_ok(H) || (depth != 8 && depth != 10)) return false;
    if (c->field < MIHEVC_CHAIN_FIELD_NONE || c->field > MIHEVC_CHAIN_FIELD_MATCH || !chain_flag_ok(c->denoise_on) || c->resize < MIHEVC_CHAIN_RESIZE_NONE ||
        c->resize > MIHEVC_CHAIN_RESIZE_SR || !chain_flag_ok(c->interpolate_on))
        return false;
    if (!c->field && !c->denoise_on && !c->resize && !c->interpolate_on) return false;
    const int sw = c->width, sh = c->height;
    if (c->field) {
        if (sh & 3) return false;
        if (c->field == MIHEVC_CHAIN_FIELD_DEINT) {
            if (!chain_flag_ok(c->deint.tff) || !chain_flag_ok(c->deint.field_rate) || !chain_zero(c->deint.reserved, 6)) return false;
        } else if (!chain_flag_ok(c->fieldmatch.tff) || !chain_flag_ok(c->fieldmatch.decimate) || !chain_flag_ok(c->fieldmatch.deint) || !chain_zero(c->fieldmatch.reserved, 5))
            return false;
    }
    if (c->denoise_on) {
        const mihevc_denoise &d = c->denoise;
        if (((d.luma_spatial | d.luma_temporal | d.chroma_spatial | d.chroma_temporal) & ~255) || !chain_zero(d.reserved, 4)) return false;
    }
    switch (c->resize) {
    case MIHEVC_CHAIN_RESIZE_NONE:
        if (sw != W || sh != H || c->bit_depth != depth) return false;
        break;
    case MIHEVC_CHAIN_RESIZE_SCALE:
        if (W > sw || sw > 4 * W || H > sh || sh > 4 * H) return false;
        break;
    case MIHEVC_CHAIN_RESIZE_UPSCALE: {
        const mihevc_upscale_src &u = c->upscale;
        if (u.width != sw || u.height != sh || u.bit_depth != c->bit_depth || u.sharpen < 0 || u.sharpen > 64 || u.antiring < 0 || u.antiring > 8 || !chain_zero(u.reserved, 3))
            return false;
        if (sw > W || W > 4 * sw || sh > H || H > 4 * sh) return false;
        break;
    }
    default: {
        const mihevc_sr_yuv &y = c->sr;
        if (sr_scale != 2 && sr_scale != 4) return false;
        if (y.width != sw || y.height != sh || y.bit_depth != c->bit_depth || !chain_matrix_ok(y.matrix) || !chain_flag_ok(y.full_range) || !chain_zero(y.reserved, 3))
            return false;
        if (!chain_matrix_ok(matrix)) return false;
        const int nw = sr_scale * sw, nh = sr_scale * sh;      // the geometry rule of mihevc_send_frame_sr_yuv
        if (!(W == nw && H == nh) && (W > nw || nw > 4 * W || H > nh || nh > 4 * H)) return false;
        break;
    }
    }
    if (c->interpolate_on) {
        const mihevc_interpolate &m = c->interpolate;
        if (m.factor < 2 || m.factor > 4 || !chain_flag_ok(m.mode) || m.scene_threshold < 0 || m.scene_threshold > 255 || !chain_zero(m.reserved, 5)) return false;
    }
    return true;
}

inline int chain_gcd(int a, int b) { return b ? chain_gcd(b, a % b) : a; }

// of a descriptor chain_check has passed
inline ChainPlan chain_plan(const mihevc_chain &c, int W, int H, int depth)
{
    ChainPlan p;
    p.field = c.field != MIHEVC_CHAIN_FIELD_NONE; p.denoise = c.denoise_on != 0; p.resize = c.resize != MIHEVC_CHAIN_RESIZE_NONE; p.interp = c.interpolate_on != 0;
    p.sw = c.width; p.sh = c.height; p.sd = c.bit_depth;
    p.dw = W; p.dh = H; p.dd = depth;
    int num = 1, den = 1;
    if (c.field == MIHEVC_CHAIN_FIELD_DEINT && c.deint.field_rate) num *= 2;
    if (c.field == MIHEVC_CHAIN_FIELD_MATCH && c.fieldmatch.decimate) { num *= 4; den *= 5; }
    if (p.interp) num *= c.interpolate.factor;
    const int g = chain_gcd(num, den);
    p.rate_num = num / g; p.rate_den = den / g;
    p.stages = (int)p.field + (int)p.denoise + (int)p.resize + (int)p.interp;
    return p;
}

// pictures that n frames give once the chain is flushed
inline int64_t chain_pictures(const mihevc_chain &c, int64_t n)
{
    if (n <= 0) return 0;
    if (c.field == MIHEVC_CHAIN_FIELD_DEINT && c.deint.field_rate) n *= 2;
    if (c.field == MIHEVC_CHAIN_FIELD_MATCH && c.fieldmatch.decimate) n -= n / 5;
    if (c.interpolate_on) n = (int64_t)c.interpolate.factor * (n - 1) + 1;
    return n;
}

}  // namespace mihevc
