"""The model of a source filter chain: nothing but the numpy models of the single filters, composed on display-size pictures in the chain's fixed
order, with the chain's numbering.  A chain is a dict with the keys of hevc_amd._lib.chain (field, tff, field_rate, decimate, fm_deint, denoise, resize, sharpen,
antiring, interpolate, interp_mode, scene_threshold) plus size=(W, H) and out_depth of the session for a resize stage.  plan() restates
hevc_amd/csrc/chain_plan.h."""
from fractions import Fraction

from tests import deint_ref, denoise_ref, fieldmatch_ref, mcfi_ref, scale_ref, upscale_ref

MODES = {"mc": 0, "blend": 1}
DEFAULTS = dict(field=None, tff=True, field_rate=False, decimate=True, fm_deint=True, denoise=None, resize=None, size=None, out_depth=None, sharpen=8, antiring=8,
                interpolate=None, interp_mode="mc", scene_threshold=10)
STAGES = ("field", "denoise", "resize", "interpolate")


def full(chain):
    assert set(chain) <= set(DEFAULTS), set(chain) - set(DEFAULTS)
    return {**DEFAULTS, **chain}


def crop(planes, w, h):
    """the display area of coded-size planes"""
    return [planes[0][:h, :w], planes[1][:h // 2, :w // 2], planes[2][:h // 2, :w // 2]]


def pictures(frames, depth, chain, with_plan=False):
    """[(pts, [Y, Cb, Cr] of the display size)] of a session whose chain is `chain`, for frames sent with pts = 0, 1, ...: picture j has pts j.  with_plan: also
    the decisions of the inverse telecine (None without one)"""
    c = full(chain)
    h, w = frames[0][0].shape
    pics, decided = [tuple(f) for f in frames], None
    if c["field"] == "deint":
        pics = [crop(p, w, h) for _, p in deint_ref.pictures(pics, depth, c["tff"], c["field_rate"])]
    elif c["field"] == "fieldmatch":
        out, decided = fieldmatch_ref.pictures(pics, depth, c["tff"], c["decimate"], c["fm_deint"])
        pics = [crop(p, w, h) for _, p in out]
    else:
        assert c["field"] is None
    if c["denoise"] is not None:
        pics = [crop(p, w, h) for _, p in denoise_ref.pictures(pics, depth, c["denoise"])]
    if c["resize"] is not None:
        (dw, dh), dd = c["size"], c["out_depth"] or depth
        if c["resize"] == "scale":
            pics = [crop(scale_ref.scale(*p, depth, dw, dh, dd), dw, dh) for p in pics]
        else:
            assert c["resize"] == "upscale"
            pics = [crop(upscale_ref.upscale(*p, depth, dw, dh, dd, c["sharpen"], c["antiring"]), dw, dh) for p in pics]
        w, h, depth = dw, dh, dd
    if c["interpolate"] is not None:
        pics = [crop(p, w, h) for p in mcfi_ref.clip_pictures(pics, depth, c["interpolate"], MODES[c["interp_mode"]], c["scene_threshold"])]
    out = list(enumerate(pics))
    return (out, decided) if with_plan else out


def without(chain, stage):
    """the chain with one of STAGES off; a chain without its resize stage stays at the source's size and depth"""
    c = dict(chain)
    c[stage] = None
    if stage == "resize":
        c.pop("size", None)
        c.pop("out_depth", None)
    return c


def stages_on(chain):
    c = full(chain)
    return [s for s in STAGES if c[s] is not None]


# ------------------------------------------------------------------------------------------------ hevc_amd/csrc/chain_plan.h, restated
def plan(chain, src, session, sr_scale=0, matrix=1, sr_matrix=6):
    """src, session: (w, h, depth).  None for a descriptor the header refuses, else dict(rate=Fraction, stages=int, sizes={stage: (w, h, depth)}, pictures=f(n)).
    resize may be 'sr' here (sr_scale: the network's scale, 0: no model)"""
    c = full(chain)
    (sw, sh, sd), (W, H, D) = src, session
    side = lambda v: 16 <= v <= 8192 and v % 2 == 0
    if not all(side(v) for v in (sw, sh, W, H)) or sd not in (8, 10) or D not in (8, 10):
        return None
    on = stages_on(c)
    if not on:
        return None
    if c["field"] is not None and sh % 4:
        return None
    if c["denoise"] is not None and any(not 0 <= v <= 255 for v in denoise_ref.strengths(c["denoise"])):
        return None
    r = c["resize"]
    if r is None and (sw, sh, sd) != (W, H, D):
        return None
    if r == "scale" and not (W <= sw <= 4 * W and H <= sh <= 4 * H):
        return None
    if r == "upscale" and not (sw <= W <= 4 * sw and sh <= H <= 4 * sh and 0 <= c["sharpen"] <= 64 and 0 <= c["antiring"] <= 8):
        return None
    if r == "sr":
        if sr_scale not in (2, 4) or matrix not in (1, 5, 6, 9) or sr_matrix not in (1, 5, 6, 9):
            return None
        nw, nh = sr_scale * sw, sr_scale * sh
        if (W, H) != (nw, nh) and not (W <= nw <= 4 * W and H <= nh <= 4 * H):
            return None
    if c["interpolate"] is not None and (c["interpolate"] not in (2, 3, 4) or c["interp_mode"] not in MODES or not 0 <= c["scene_threshold"] <= 255):
        return None
    rate = Fraction(1)
    if c["field"] == "deint" and c["field_rate"]:
        rate *= 2
    if c["field"] == "fieldmatch" and c["decimate"]:
        rate *= Fraction(4, 5)
    if c["interpolate"] is not None:
        rate *= c["interpolate"]

    def count(n):
        if n <= 0:
            return 0
        if c["field"] == "deint" and c["field_rate"]:
            n *= 2
        if c["field"] == "fieldmatch" and c["decimate"]:
            n -= n // 5
        return c["interpolate"] * (n - 1) + 1 if c["interpolate"] is not None else n

    sizes = {s: ((sw, sh, sd) if s in ("field", "denoise") else (W, H, D)) for s in on}
    return dict(rate=rate, stages=len(on), sizes=sizes, pictures=count)
