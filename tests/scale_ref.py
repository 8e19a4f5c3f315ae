"""numpy model of the downscaling source (mihevc_send_frame_scaled / mihevc_k_scale_source), written from the definition of DESIGN.md §6e alone; imports nothing
from hevc_amd.  Coefficients come from fractions.Fraction, the filters are one gather-and-accumulate per tap.

Source: planar 4:2:0, sw x sh, B significant bits (uint8 at B == 8, else little-endian uint16, lsb aligned, values above 2^B - 1 clamped).  Output: dw x dh at D
bits, dst <= src <= 4 dst per axis, in planes of the coded size (rounded up to 8).  One axis of one plane, S source and Dn output samples, r = S / Dn, p = 2
(centre aligned: luma, and chroma vertically) or 1 (chroma horizontally, co-sited with the even luma column):
  position   pos = ((4i + p) S - p Dn) / (4 Dn)
  taps       every integer k with |pos - k| < 2r
  weight     w_k = CR((pos - k) / r): CR(t) = 1.5|t|^3 - 2.5|t|^2 + 1 for |t| <= 1, -0.5|t|^3 + 2.5|t|^2 - 4|t| + 2 for 1 < |t| < 2
  coefficient  c_k = floor(w_k 4096 / sum(w) + 1/2); 4096 - sum(c) is added to the largest c_k (the lowest k among equals); coefficients that are 0 at
               either end of the row are then dropped (1:1 is the single tap 4096)
  source index  k is clamped to [0, S - 1] when the sample is read
  horizontal first  m = floor((sum c_k v_k + 2^(11-G)) / 2^(12-G)), G = min(4, 16 - B)
  vertical on m     T = sum c_k m_k, n = 12 + G + max(0, B - D), u = max(0, D - B), out = clamp(floor((T 2^u + 2^(n-1)) / 2^n), 0, 2^D - 1)
  margin     outside the display area: the output sample at (min(x, dw - 1), min(y, dh - 1))
"""
import functools
import math
from fractions import Fraction

import numpy as np

TAPS = 16
ONE = 4096


def coded(n):
    return (n + 7) // 8 * 8


def cr(t):
    t = abs(t)
    if t <= 1:
        return Fraction(3, 2) * t ** 3 - Fraction(5, 2) * t ** 2 + 1
    if t < 2:
        return -Fraction(1, 2) * t ** 3 + Fraction(5, 2) * t ** 2 - 4 * t + 2
    return Fraction(0)


def row(pos, r):
    """(first k, coefficients) of the output sample at `pos`"""
    lo, hi = math.floor(pos - 2 * r) + 1, math.ceil(pos + 2 * r) - 1          # the integers strictly inside (pos - 2r, pos + 2r)
    w = [cr((pos - k) / r) for k in range(lo, hi + 1)]
    total = sum(w)
    c = [math.floor(x * ONE / total + Fraction(1, 2)) for x in w]
    c[c.index(max(c))] += ONE - sum(c)
    while len(c) > 1 and c[0] == 0:                   # coefficients that came out 0 at either end are dropped
        lo, c = lo + 1, c[1:]
    while len(c) > 1 and c[-1] == 0:
        c = c[:-1]
    return lo, c


@functools.lru_cache(maxsize=None)
def table(S, Dn, p):
    """(first[Dn] int32, coef[Dn, 16] int16 zero padded, length of the longest row) of one axis"""
    assert Dn <= S <= 4 * Dn and p in (1, 2)
    r = Fraction(S, Dn)
    first, coef = np.zeros(Dn, np.int32), np.zeros((Dn, TAPS), np.int16)
    longest, phases = 0, {}
    for i in range(Dn):
        pos = Fraction((4 * i + p) * S - p * Dn, 4 * Dn)
        base = math.floor(pos)
        frac = pos - base
        if frac not in phases:                        # the weights depend on the fractional part of pos alone
            lo, c = row(frac, r)
            assert len(c) <= TAPS
            phases[frac] = (lo, c)
        lo, c = phases[frac]
        first[i] = base + lo
        coef[i, :len(c)] = c
        longest = max(longest, len(c))
    return first, coef, longest


def src_dtype(B):
    return np.uint8 if B == 8 else np.dtype("<u2")


def out_dtype(D):
    return np.uint8 if D == 8 else np.uint16


def filter_axis(x, S, Dn, p, axis):
    """sum_k c_k x[clamp(k)] along `axis` (int64): one gather and one multiply-accumulate per tap"""
    first, coef, longest = table(S, Dn, p)
    x = np.moveaxis(x, axis, -1)
    assert x.shape[-1] == S
    acc = np.zeros(x.shape[:-1] + (Dn,), np.int64)
    for j in range(longest):
        acc += coef[:, j].astype(np.int64) * x[..., np.clip(first.astype(np.int64) + j, 0, S - 1)]
    return np.moveaxis(acc, -1, axis)


def scale_plane(v, B, D, dw, dh, ph_, pv):
    """one plane of sample values (int64, already clamped) -> dw x dh output samples"""
    sh, sw = v.shape
    G = min(4, 16 - B)
    m = (filter_axis(v, sw, dw, ph_, 1) + (1 << (11 - G))) >> (12 - G)
    T = filter_axis(m, sh, dh, pv, 0)
    n, u = 12 + G + max(0, B - D), max(0, D - B)
    return np.clip((T * (1 << u) + (1 << (n - 1))) >> n, 0, (1 << D) - 1)


def scale(y, u, v, B, dw, dh, D):
    """source planes (sh x sw, and halves) at B bits -> (Y, Cb, Cr) of the coded size of dw x dh at D bits"""
    sh, sw = y.shape
    assert sw % 2 == 0 and sh % 2 == 0 and dw % 2 == 0 and dh % 2 == 0 and u.shape == v.shape == (sh // 2, sw // 2)
    pw, ph = coded(dw), coded(dh)
    out = []
    for c, pl in enumerate((y, u, v)):
        val = np.minimum(np.asarray(pl).astype(np.int64), (1 << B) - 1)
        w, h, cw, chh = (dw, dh, pw, ph) if c == 0 else (dw // 2, dh // 2, pw // 2, ph // 2)
        o = scale_plane(val, B, D, w, h, 2 if c == 0 else 1, 2)
        out.append(np.ascontiguousarray(np.pad(o, ((0, chh - h), (0, cw - w)), mode="edge").astype(out_dtype(D))))
    return out


def random_source(sw, sh, B, seed, full_word=False):
    """uniform random full-range planes (y, u, v); full_word: deeper than 8 bit with values above the declared depth, which the definition clamps"""
    rng = np.random.default_rng(seed)
    top = 1 << (16 if (full_word and B > 8) else B)
    return [np.ascontiguousarray(rng.integers(0, top, s).astype(src_dtype(B))) for s in ((sh, sw), (sh // 2, sw // 2), (sh // 2, sw // 2))]
