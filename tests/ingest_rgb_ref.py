"""numpy model of the RGB source conversion (mihevc_send_frame_rgb / mihevc_k_convert_rgb), written from the definition alone; imports nothing from hevc_amd.

A source picture is W x H (display size, both even), full-range R'G'B'.  B = significant bits of a source sample (8 .. 16, lsb aligned), D = bit depth of the
output (8 or 10).
  sample   integers: raw element r (uint8 at B == 8, else little-endian uint16), v = min(r, 2^B - 1).  Floats (IEEE half or single, planar only): B = 16 and
           v = rint(min(max(x, 0), 1) * 65535): a half is widened to float32 exactly, the product is one float32 multiplication rounded to nearest even, rint
           is ties-to-even, NaN gives 0
  matrix   code 1 (BT.709), 5 or 6 (BT.601), 9 (BT.2020 ncl): (Kr, Kb) in 1/10000 = (2126, 722), (2990, 1140), (2627, 593), Kg = 1 - Kr - Kb.
           Y row (Kr, Kg, Kb); Cb row (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb)); Cr row (1 - Kr, -Kg, -Kb) / (2 (1 - Kr))
  scale    limited: sY = 219 2^(D-8) / (2^B - 1), sC = 224 2^(D-8) / (2^B - 1), oY = 16 2^(D-8); full: sY = sC = (2^D - 1) / (2^B - 1), oY = 0; oC = 2^(D-1)
  coefficients  S = 16 + max(0, B - D); m[r][c] = floor(row[r][c] s 2^S + 1/2), exactly (fractions.Fraction)
  pixel    t[r] = m[r][0] R + m[r][1] G + m[r][2] B (64 bits)
  luma     Y = clip(((t[0] + 2^(S-1)) >> S) + oY, 0, 2^D - 1)
  chroma   output (i, j): T = sum over rows {2j, 2j+1} of t[c] at column max(2i-1, 0) + 2 t[c] at column 2i + t[c] at column 2i+1;
           C = clip(((T + 2^(S+2)) >> (S+3)) + oC, 0, 2^D - 1); shifts of negative values floor
  margin   the output planes have the coded size (display size rounded up to 8); a sample outside the display area equals the output sample at
           (min(x, sw - 1), min(y, sh - 1))
"""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

# layout: 0 three planes, 3 / 4 packed; r, g, b: the component's plane / element index; sample: 0 integer, 1 half, 2 single; bit_depth: 8 .. 16 (floats: 0)
Format = namedtuple("Format", "layout r g b sample bit_depth")

# ffmpeg pixel format names the conversion covers
FORMATS = {"gbrp": Format(0, 2, 0, 1, 0, 8), "gbrpf32le": Format(0, 2, 0, 1, 2, 0),
           "rgb24": Format(3, 0, 1, 2, 0, 8), "bgr24": Format(3, 2, 1, 0, 0, 8),
           "rgb48le": Format(3, 0, 1, 2, 0, 16), "bgr48le": Format(3, 2, 1, 0, 0, 16), "rgba64le": Format(4, 0, 1, 2, 0, 16), "bgra64le": Format(4, 2, 1, 0, 0, 16)}
for _b in (9, 10, 12, 14, 16):
    FORMATS[f"gbrp{_b}le"] = Format(0, 2, 0, 1, 0, _b)
for _names, _rgb in ((("rgba", "rgb0"), (0, 1, 2)), (("bgra", "bgr0"), (2, 1, 0)), (("argb", "0rgb"), (1, 2, 3)), (("abgr", "0bgr"), (3, 2, 1))):
    for _n in _names:
        FORMATS[_n] = Format(4, *_rgb, 0, 8)
UNSUPPORTED = ("gbrp10be", "rgb48be", "gbrap", "gbrap10le", "gbrapf32le", "rgb565le", "rgb565be", "x2rgb10le", "pal8", "gray", "gray10le", "gbrpf32be", "yuv420p", "nv12")

MATRICES = {1: (2126, 722), 5: (2990, 1140), 6: (2990, 1140), 9: (2627, 593)}


def coded(n):
    return (n + 7) // 8 * 8


def depth_of(f):
    return 16 if f.sample else f.bit_depth


def src_dtype(f):
    if f.sample:
        return np.dtype("<f2") if f.sample == 1 else np.dtype("<f4")
    return np.dtype(np.uint8) if f.bit_depth == 8 else np.dtype("<u2")


def out_dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def plane_shapes(f, w, h):
    """shapes of the source arrays: three (h, w) planes, or one packed (h, layout * w) plane"""
    return [(h, w)] * 3 if f.layout == 0 else [(h, f.layout * w)]


def rows(matrix):
    """the three rows of the matrix as Fractions"""
    kr, kb = (Fraction(k, 10000) for k in MATRICES[matrix])
    kg = 1 - kr - kb
    return [[kr, kg, kb], [x / (2 * (1 - kb)) for x in (-kr, -kg, 1 - kb)], [x / (2 * (1 - kr)) for x in (1 - kr, -kg, -kb)]]


def scales(full, B, D):
    """(sY, sC, oY, oC)"""
    top = (1 << B) - 1
    if full:
        return Fraction((1 << D) - 1, top), Fraction((1 << D) - 1, top), 0, 1 << (D - 1)
    return Fraction(219 << (D - 8), top), Fraction(224 << (D - 8), top), 16 << (D - 8), 1 << (D - 1)


def coefficients(matrix, full, B, D):
    """(m, S): m[r][c] = floor(row[r][c] s 2^S + 1/2)"""
    S = 16 + max(0, B - D)
    sy, sc, _, _ = scales(full, B, D)
    return [[math.floor(x * (sc if r else sy) * (1 << S) + Fraction(1, 2)) for x in row] for r, row in enumerate(rows(matrix))], S


def sample(x, f):
    """raw elements -> sample values (int64)"""
    x = np.asarray(x)
    if f.sample:
        x = x.astype(np.float32)                              # exact for a half, subnormals included
        x = np.where(x > 0, x, np.float32(0))                 # NaN compares false: 0
        x = np.where(x < 1, x, np.float32(1)).astype(np.float32)
        return np.rint(x * np.float32(65535)).astype(np.int64)
    return np.minimum(x.astype(np.int64), (1 << f.bit_depth) - 1)


def components(f, planes):
    """(R, G, B) sample values, (h, w) each"""
    if f.layout == 0:
        return [sample(planes[i], f) for i in (f.r, f.g, f.b)]
    p = sample(planes[0], f)
    return [p[:, i::f.layout] for i in (f.r, f.g, f.b)]


def pad(out, ph, pw, depth):
    h, w = out.shape
    return np.ascontiguousarray(np.pad(out, ((0, ph - h), (0, pw - w)), mode="edge").astype(out_dtype(depth)))


def convert(f, planes, matrix, full, depth):
    """source planes (display size) -> (Y, Cb, Cr) of the coded size at `depth` bits"""
    rgb = components(f, planes)
    h, w = rgb[0].shape
    assert w % 2 == 0 and h % 2 == 0
    m, S = coefficients(matrix, full, depth_of(f), depth)
    _, _, oy, oc = scales(full, depth_of(f), depth)
    peak, pw, ph = (1 << depth) - 1, coded(w), coded(h)
    t = [m[r][0] * rgb[0] + m[r][1] * rgb[1] + m[r][2] * rgb[2] for r in range(3)]
    out = [pad(np.clip(((t[0] + (1 << (S - 1))) >> S) + oy, 0, peak), ph, pw, depth)]
    for c in t[1:]:
        left = np.concatenate([c[:, :1], c[:, 1:-1:2]], axis=1)            # column max(2i - 1, 0)
        hsum = left + 2 * c[:, 0::2] + c[:, 1::2]
        T = hsum[0::2] + hsum[1::2]
        out.append(pad(np.clip(((T + (1 << (S + 2))) >> (S + 3)) + oc, 0, peak), ph // 2, pw // 2, depth))
    return out


def random_source(f, w, h, seed, full_word=False):
    """uniform random samples in the source layout (plane_shapes).  Integer planes deeper than 8 bit also get values above the declared depth (full_word), which
    the conversion clamps; float planes run from -0.25 to 1.25 and hold a NaN, an infinity and a negative zero"""
    rng = np.random.default_rng(seed)
    dt = src_dtype(f)
    out = []
    for s in plane_shapes(f, w, h):
        if f.sample:
            p = (rng.random(s) * 1.5 - 0.25).astype(dt)
            p[0, 1], p[1, 0], p[1, 2], p[2, 2] = np.nan, np.inf, -0.0, -np.inf
        else:
            p = rng.integers(0, 1 << (16 if full_word and f.bit_depth > 8 else f.bit_depth), s).astype(dt)
        out.append(np.ascontiguousarray(p))
    return out
