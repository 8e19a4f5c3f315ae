"""numpy model of the source conversion (mihevc_send_frame_fmt / mihevc_k_convert_source), written from the definition alone; imports nothing from hevc_amd.

A source picture is W x H (display size, both even); its chroma planes are W/2 x H/2 (420), W/2 x H (422) or W x H (444).  B = significant bits of a source
sample (8 .. 16), D = bit depth of the output (8 or 10).
  sample   raw element r (uint8 at B == 8, else little-endian uint16): msb_aligned: v = r >> (16 - B); otherwise v = min(r, 2^B - 1)
  chroma   output sample (i, j): 420 S = c[j][i], k = 0; 422 S = c[2j][i] + c[2j+1][i], k = 1;
           444 S = sum over r in {2j, 2j+1} of (c[r][max(2i-1, 0)] + 2 c[r][2i] + c[r][2i+1]), k = 3.  Luma: S = v, k = 0
  depth    n = k + max(0, B - D), m = max(0, D - B); out = min(((S << m) + ((1 << n) >> 1)) >> n, 2^D - 1)
  margin   the output planes have the coded size (display size rounded up to 8); a sample outside the display area equals the output sample at
           (min(x, sw - 1), min(y, sh - 1))
  semi-planar  u holds Cb in its even and Cr in its odd elements; v is ignored
"""
from collections import namedtuple

import numpy as np

Format = namedtuple("Format", "chroma semi_planar bit_depth msb_aligned")

# ffmpeg pixel format names the conversion covers
FORMATS = {}
for _c in (420, 422, 444):
    FORMATS[f"yuv{_c}p"] = Format(_c, 0, 8, 0)
    FORMATS[f"yuvj{_c}p"] = Format(_c, 0, 8, 0)
    for _b in (9, 10, 12, 14, 16):
        FORMATS[f"yuv{_c}p{_b}le"] = Format(_c, 0, _b, 0)
FORMATS.update({"nv12": Format(420, 1, 8, 0), "nv16": Format(422, 1, 8, 0), "nv24": Format(444, 1, 8, 0),
                "p010le": Format(420, 1, 10, 1), "p016le": Format(420, 1, 16, 1), "p210le": Format(422, 1, 10, 1), "p216le": Format(422, 1, 16, 1),
                "p410le": Format(444, 1, 10, 1), "p416le": Format(444, 1, 16, 1)})
UNSUPPORTED = ("nv21", "yuyv422", "gbrp", "yuv411p", "yuv420p10be")


def coded(n):
    return (n + 7) // 8 * 8


def src_dtype(f):
    return np.uint8 if f.bit_depth == 8 else np.dtype("<u2")


def out_dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def plane_shapes(f, w, h):
    """shapes of the source arrays (y, u, v); semi-planar: u is the interleaved plane, v is None"""
    cw, ch = (w if f.chroma == 444 else w // 2), (h // 2 if f.chroma == 420 else h)
    return ((h, w), (ch, 2 * cw), None) if f.semi_planar else ((h, w), (ch, cw), (ch, cw))


def sample(r, f):
    r = np.asarray(r).astype(np.int64)
    return r >> (16 - f.bit_depth) if f.msb_aligned else np.minimum(r, (1 << f.bit_depth) - 1)


def chroma_sum(c, chroma):
    """(S, k) of a chroma plane of sample values"""
    if chroma == 420:
        return c, 0
    if chroma == 422:
        return c[0::2] + c[1::2], 1
    left = np.concatenate([c[:, :1], c[:, 1:-1:2]], axis=1)            # column max(2i - 1, 0)
    hsum = left + 2 * c[:, 0::2] + c[:, 1::2]
    return hsum[0::2] + hsum[1::2], 3


def finish(S, k, f, depth, pw, ph):
    n, m = k + max(0, f.bit_depth - depth), max(0, depth - f.bit_depth)
    out = np.minimum(((S << m) + ((1 << n) >> 1)) >> n, (1 << depth) - 1)
    h, w = out.shape
    return np.ascontiguousarray(np.pad(out, ((0, ph - h), (0, pw - w)), mode="edge").astype(out_dtype(depth)))


def convert(f, y, u, v, depth):
    """source planes (display size) -> (Y, Cb, Cr) of the coded size at `depth` bits"""
    h, w = y.shape
    assert w % 2 == 0 and h % 2 == 0
    pw, ph = coded(w), coded(h)
    if f.semi_planar:
        u, v = u[:, 0::2], u[:, 1::2]
    out = [finish(sample(y, f), 0, f, depth, pw, ph)]
    for c in (u, v):
        S, k = chroma_sum(sample(c, f), f.chroma)
        assert S.shape == (h // 2, w // 2)
        out.append(finish(S, k, f, depth, pw // 2, ph // 2))
    return out


def random_source(f, w, h, seed, full_word=False):
    """uniform random full-range samples in the source layout: (y, u, v) as plane_shapes.  lsb-aligned planes deeper than 8 bit also get values above the
    declared depth (full_word), which the conversion clamps; msb-aligned ones random low bits, which it drops"""
    rng = np.random.default_rng(seed)
    dt = src_dtype(f)
    top = 1 << (16 if (f.msb_aligned or (full_word and f.bit_depth > 8)) else f.bit_depth)
    return [None if s is None else np.ascontiguousarray(rng.integers(0, top, s).astype(dt)) for s in plane_shapes(f, w, h)]
