"""numpy model of the upscaling source (mihevc_send_frame_upscaled / mihevc_k_upscale_source), written from the definition of DESIGN.md §6k alone; imports nothing
from hevc_amd.  Coefficients come from fractions.Fraction, the filters are one gather-and-accumulate per tap.

Source: planar 4:2:0, sw x sh, B significant bits (uint8 at B == 8, else little-endian uint16, values above 2^B - 1 clamped).  Output: dw x dh at D bits,
src <= dst <= 4 src per axis, in planes of the coded size (rounded up to 8).  One axis of one plane, S source and Dn output samples, p = 2 (centre aligned:
luma, and chroma vertically) or 1 (chroma horizontally, co-sited):
  position   pos = ((4i + p) S - p Dn) / (4 Dn), near = floor(pos)
  taps       every integer k with |pos - k| < 2, weight CR(pos - k)
  coefficient  c_k = floor(w_k 4096 / sum(w) + 1/2); 4096 - sum(c) is added to the largest c_k (the lowest k among equals); zeros at either end dropped
  horizontal  m = floor((sum c_k v_k + 2^(11-G)) / 2^(12-G)), G = min(4, 16 - B); k clamped to the plane when read
  anti-ringing  a, b = v[near], v[near + 1] (clamped into the plane), lo = min(a, b) 2^G, hi = max(a, b) 2^G, m' = m + floor(((clamp(m, lo, hi) - m) ar + 4) / 8)
  vertical on m'  t = floor((sum c_k m'_k + 2^11) / 2^12), t' = t blended the same way against m' of rows near, near + 1 (no further scaling)
  output     P = clamp(floor((t' 2^u + 2^(n-1)) / 2^n), 0, 2^D - 1), n = G + max(0, B - D), u = max(0, D - B)
  sharpening  luma only, on P inside the display area, neighbours clamped into it: e = the four edge neighbours, f = the four corners,
              d16 = 16 c - (4 c + 2 e + f), q = c + floor((d16 g + 128) / 256), out = clamp(q, min3x3, max3x3)
  margin     outside the display area: the output sample at (min(x, dw - 1), min(y, dh - 1))
"""
import functools
import math
from fractions import Fraction

import numpy as np

from tests.scale_ref import coded, cr, out_dtype, random_source, src_dtype      # noqa: F401 (the element types, the cubic and the sources are the downscaler's)

TAPS = 4
ONE = 4096


def row(pos):
    """(first k, coefficients) of the output sample at `pos`"""
    lo, hi = math.floor(pos - 2) + 1, math.ceil(pos + 2) - 1            # the integers strictly inside (pos - 2, pos + 2)
    w = [cr(pos - k) for k in range(lo, hi + 1)]
    total = sum(w)
    c = [math.floor(x * ONE / total + Fraction(1, 2)) for x in w]
    c[c.index(max(c))] += ONE - sum(c)
    while len(c) > 1 and c[0] == 0:
        lo, c = lo + 1, c[1:]
    while len(c) > 1 and c[-1] == 0:
        c = c[:-1]
    return lo, c


@functools.lru_cache(maxsize=None)
def table(S, Dn, p):
    """(first[Dn] int32, near[Dn] int32, coef[Dn, 4] int16 zero padded, length of the longest row) of one axis"""
    assert S <= Dn <= 4 * S and p in (1, 2)
    first, near, coef = np.zeros(Dn, np.int32), np.zeros(Dn, np.int32), np.zeros((Dn, TAPS), np.int16)
    longest, phases = 0, {}
    for i in range(Dn):
        pos = Fraction((4 * i + p) * S - p * Dn, 4 * Dn)
        base = math.floor(pos)
        frac = pos - base
        if frac not in phases:
            phases[frac] = row(frac)
        lo, c = phases[frac]
        assert len(c) <= TAPS
        first[i], near[i] = base + lo, base
        coef[i, :len(c)] = c
        longest = max(longest, len(c))
    return first, near, coef, longest


def filter_axis(x, S, Dn, p, axis):
    """sum_k c_k x[clamp(k)] along `axis` (int64)"""
    first, _, coef, longest = table(S, Dn, p)
    x = np.moveaxis(x, axis, -1)
    assert x.shape[-1] == S
    acc = np.zeros(x.shape[:-1] + (Dn,), np.int64)
    for j in range(longest):
        acc += coef[:, j].astype(np.int64) * x[..., np.clip(first.astype(np.int64) + j, 0, S - 1)]
    return np.moveaxis(acc, -1, axis)


def blend_to_range(m, x, S, Dn, p, axis, scale, ar):
    """m blended, ar eighths of the way, into the range of the two samples of x (times `scale`) that lie around each output position along `axis`"""
    near = table(S, Dn, p)[1].astype(np.int64)
    x = np.moveaxis(x, axis, -1)
    a, b = x[..., np.clip(near, 0, S - 1)] * scale, x[..., np.clip(near + 1, 0, S - 1)] * scale
    m = np.moveaxis(m, axis, -1)
    out = m + (((np.clip(m, np.minimum(a, b), np.maximum(a, b)) - m) * ar + 4) >> 3)
    return np.moveaxis(out, -1, axis)


def interpolate_plane(v, B, D, dw, dh, ph_, pv, ar):
    """one plane of sample values (int64, already clamped) -> the dw x dh samples P"""
    sh, sw = v.shape
    G = min(4, 16 - B)
    m = (filter_axis(v, sw, dw, ph_, 1) + (1 << (11 - G))) >> (12 - G)
    m = blend_to_range(m, v, sw, dw, ph_, 1, 1 << G, ar)
    t = (filter_axis(m, sh, dh, pv, 0) + (1 << 11)) >> 12
    t = blend_to_range(t, m, sh, dh, pv, 0, 1, ar)
    n, u = G + max(0, B - D), max(0, D - B)
    return np.clip((t * (1 << u) + (1 << (n - 1))) >> n, 0, (1 << D) - 1)


def sharpen_plane(P, g):
    """the limited 3x3 sharpener on a plane of P (neighbours clamped into it), gain g sixteenths"""
    h, w = P.shape
    q = np.pad(P.astype(np.int64), 1, mode="edge")
    win = [q[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)]
    c = win[4]
    e, f = win[1] + win[3] + win[5] + win[7], win[0] + win[2] + win[6] + win[8]
    d16 = 16 * c - (4 * c + 2 * e + f)
    return np.clip(c + ((d16 * g + 128) >> 8), np.minimum.reduce(win), np.maximum.reduce(win))


def interpolate(y, u, v, B, dw, dh, D, ar):
    """the three planes P of the display size (int64), before sharpening"""
    out = []
    for c, pl in enumerate((y, u, v)):
        val = np.minimum(np.asarray(pl).astype(np.int64), (1 << B) - 1)
        w, h = (dw, dh) if c == 0 else (dw // 2, dh // 2)
        out.append(interpolate_plane(val, B, D, w, h, 2 if c == 0 else 1, 2, ar))
    return out


def upscale(y, u, v, B, dw, dh, D, sharpen=8, antiring=8):
    """source planes (sh x sw, and halves) at B bits -> (Y, Cb, Cr) of the coded size of dw x dh at D bits"""
    sh, sw = y.shape
    assert sw % 2 == 0 and sh % 2 == 0 and dw % 2 == 0 and dh % 2 == 0 and u.shape == v.shape == (sh // 2, sw // 2)
    assert 0 <= sharpen <= 64 and 0 <= antiring <= 8
    pw, ph = coded(dw), coded(dh)
    P = interpolate(y, u, v, B, dw, dh, D, antiring)
    P[0] = sharpen_plane(P[0], sharpen)
    out = []
    for c, o in enumerate(P):
        w, h, cw, chh = (dw, dh, pw, ph) if c == 0 else (dw // 2, dh // 2, pw // 2, ph // 2)
        out.append(np.ascontiguousarray(np.pad(o, ((0, chh - h), (0, cw - w)), mode="edge").astype(out_dtype(D))))
    return out
