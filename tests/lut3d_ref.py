"""numpy model of the colour table source (mihevc_send_frame_lut3d / mihevc_k_lut3d), written from DESIGN.md §6i (and §6d for its last step) alone; imports nothing
from hevc_amd and shares nothing with the kernel header.

A picture is W x H (display size, both even), planar 4:2:0 Y'CbCr at B = 8, 10 or 12 bit (v = min(r, 2^B - 1)), matrix code 1, 5, 6 or 9, limited or full range.
The output is planar 4:2:0 at D = 8 or 10 with a matrix and range of its own, planes of the coded size.  Integers throughout; shifts of negative values floor.
  1 chroma to the luma grid, factor 8, no rounding: h(i, 2x) = 2 c[i][x], h(i, 2x+1) = c[i][x] + c[i][min(x+1, W/2-1)];
    row 2j: C8 = 3 h(j) + h(max(j-1, 0)); row 2j+1: C8 = 3 h(j) + h(min(j+1, H/2-1))
  2 y = Y - oY, cb = Cb8 - 8 oC, cr = Cr8 - 8 oC; five coefficients n = floor(coef 2^16 + 1/2): nY = sY, nRv = 2(1-Kr) sC / 8, nGu = -(2 Kb (1-Kb) / Kg) sC / 8,
    nGv = -(2 Kr (1-Kr) / Kg) sC / 8, nBu = 2(1-Kb) sC / 8; v = clip((t + 2^15) >> 16, 0, 65535) for t_R = nY y + nRv cr, t_G = nY y + nGu cb + nGv cr,
    t_B = nY y + nBu cb
  3 p = v (N-1), i = min(p // 65535, N-2), f = p - 65535 i; fractions sorted f1 >= f2 >= f3 with axes a1, a2, a3; V0 = L[i], V1 = V0 + a1, V2 = V1 + a2,
    V3 = V0 + all three; o = ((65535 - f1) V0 + (f1 - f2) V1 + (f2 - f3) V2 + f3 V3 + 32767) // 65535
  4 §6d with B = 16 from "matrix" on
"""
import math
from fractions import Fraction

import numpy as np

MATRICES = {1: (2126, 722), 5: (2990, 1140), 6: (2990, 1140), 9: (2627, 593)}


def coded(n):
    return (n + 7) // 8 * 8


def dtype(depth):
    return np.dtype(np.uint8) if depth == 8 else np.dtype("<u2")


# ------------------------------------------------------------------------------------------------ step 1
def chroma_to_luma_grid(c):
    """(H/2, W/2) samples -> (H, W) int64 with the factor 8"""
    c = np.asarray(c, np.int64)
    right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    h = np.empty((c.shape[0], 2 * c.shape[1]), np.int64)
    h[:, 0::2] = 2 * c
    h[:, 1::2] = c + right
    up = np.concatenate([h[:1], h[:-1]])
    down = np.concatenate([h[1:], h[-1:]])
    out = np.empty((2 * h.shape[0], h.shape[1]), np.int64)
    out[0::2] = 3 * h + up
    out[1::2] = 3 * h + down
    return out


# ------------------------------------------------------------------------------------------------ step 2
def inverse_coefficients(matrix, full, B):
    """(nY, nRv, nGu, nGv, nBu)"""
    kr, kb = (Fraction(k, 10000) for k in MATRICES[matrix])
    kg = 1 - kr - kb
    if full:
        sy = sc = Fraction(65535, (1 << B) - 1)
    else:
        sy, sc = Fraction(65535, 219 << (B - 8)), Fraction(65535, 224 << (B - 8))
    coefs = [sy, 2 * (1 - kr) * sc / 8, -(2 * kb * (1 - kb) / kg) * sc / 8, -(2 * kr * (1 - kr) / kg) * sc / 8, 2 * (1 - kb) * sc / 8]
    return tuple(math.floor(c * 65536 + Fraction(1, 2)) for c in coefs)


def unclipped_rgb16(Y, cb8, cr8, matrix, full, B):
    """the three (t + 2^15) >> 16 before the clip, int64"""
    ny, nrv, ngu, ngv, nbu = inverse_coefficients(matrix, full, B)
    y = np.asarray(Y, np.int64) - (0 if full else 16 << (B - 8))
    cb = np.asarray(cb8, np.int64) - (8 << (B - 1))
    cr = np.asarray(cr8, np.int64) - (8 << (B - 1))
    t = (ny * y + nrv * cr, ny * y + ngu * cb + ngv * cr, ny * y + nbu * cb)
    return [(x + (1 << 15)) >> 16 for x in t]


def to_rgb16(Y, cb8, cr8, matrix, full, B):
    return [np.clip(x, 0, 65535) for x in unclipped_rgb16(Y, cb8, cr8, matrix, full, B)]


def in_gamut(Y, cb, cr, matrix, full, B):
    """of flat colours (Y, Cb, Cr samples, not 8-fold): those whose R'G'B' of step 2 needs no clipping"""
    u = unclipped_rgb16(Y, 8 * np.asarray(cb, np.int64), 8 * np.asarray(cr, np.int64), matrix, full, B)
    return np.logical_and.reduce([(x >= 0) & (x <= 65535) for x in u])


# ------------------------------------------------------------------------------------------------ step 3
def lookup(table, rgb):
    """table: (N, N, N, 3) uint16 indexed [b][g][r][c]; rgb: three int64 arrays of 0 .. 65535 -> three int64 arrays"""
    table = np.asarray(table)
    N = table.shape[0]
    assert table.shape == (N, N, N, 3) and 2 <= N <= 65
    L = table.astype(np.int64)
    shape = np.shape(rgb[0])
    v = np.stack([np.asarray(x, np.int64).ravel() for x in rgb], axis=1)          # (n, 3): r, g, b
    p = v * (N - 1)
    i = np.minimum(p // 65535, N - 2)
    f = p - 65535 * i
    assert f.min() >= 0 and f.max() <= 65535
    order = np.argsort(-f, axis=1, kind="stable")                                # axes by falling fraction
    fs = np.take_along_axis(f, order, axis=1)
    f1, f2, f3 = fs[:, 0], fs[:, 1], fs[:, 2]
    n = len(v)
    rows = np.arange(n)
    pos = i.copy()
    V = [L[pos[:, 2], pos[:, 1], pos[:, 0]]]
    for k in (0, 1, 2):
        pos[rows, order[:, k]] += 1
        V.append(L[pos[:, 2], pos[:, 1], pos[:, 0]])
    w = [65535 - f1, f1 - f2, f2 - f3, f3]
    acc = sum(wk[:, None] * Vk for wk, Vk in zip(w, V)) + 32767
    assert acc.max() < 1 << 32
    o = acc // 65535
    return [o[:, c].reshape(shape) for c in range(3)]


# ------------------------------------------------------------------------------------------------ step 4 (§6d, B = 16)
def forward_coefficients(matrix, full, D):
    """(m, S, oY, oC) for 16-bit R'G'B'"""
    kr, kb = (Fraction(k, 10000) for k in MATRICES[matrix])
    kg = 1 - kr - kb
    rows = [[kr, kg, kb], [x / (2 * (1 - kb)) for x in (-kr, -kg, 1 - kb)], [x / (2 * (1 - kr)) for x in (1 - kr, -kg, -kb)]]
    S = 16 + 16 - D
    if full:
        sy = sc = Fraction((1 << D) - 1, 65535)
        oy = 0
    else:
        sy, sc, oy = Fraction(219 << (D - 8), 65535), Fraction(224 << (D - 8), 65535), 16 << (D - 8)
    m = [[math.floor(x * (sc if r else sy) * (1 << S) + Fraction(1, 2)) for x in row] for r, row in enumerate(rows)]
    return m, S, oy, 1 << (D - 1)


def pad(out, ph, pw, depth):
    h, w = out.shape
    return np.ascontiguousarray(np.pad(out, ((0, ph - h), (0, pw - w)), mode="edge").astype(dtype(depth)))


def from_rgb16(rgb, matrix, full, D):
    """three (H, W) int64 arrays -> (Y, Cb, Cr) of the coded size"""
    h, w = rgb[0].shape
    m, S, oy, oc = forward_coefficients(matrix, full, D)
    peak, pw, ph = (1 << D) - 1, coded(w), coded(h)
    t = [m[r][0] * rgb[0] + m[r][1] * rgb[1] + m[r][2] * rgb[2] for r in range(3)]
    out = [pad(np.clip(((t[0] + (1 << (S - 1))) >> S) + oy, 0, peak), ph, pw, D)]
    for c in t[1:]:
        left = np.concatenate([c[:, :1], c[:, 1:-1:2]], axis=1)
        hsum = left + 2 * c[:, 0::2] + c[:, 1::2]
        T = hsum[0::2] + hsum[1::2]
        out.append(pad(np.clip(((T + (1 << (S + 2))) >> (S + 3)) + oc, 0, peak), ph // 2, pw // 2, D))
    return out


# ------------------------------------------------------------------------------------------------ the whole
def convert(planes, B, matrix, full, table, D, out_matrix, out_full):
    """(Y, Cb, Cr) source planes of the display size -> (Y, Cb, Cr) of the coded size at D bits"""
    peak = (1 << B) - 1
    Y, cb, cr = (np.minimum(np.asarray(p, np.int64), peak) for p in planes)
    assert Y.shape[0] % 2 == 0 and Y.shape[1] % 2 == 0 and cb.shape == cr.shape == (Y.shape[0] // 2, Y.shape[1] // 2)
    rgb = to_rgb16(Y, chroma_to_luma_grid(cb), chroma_to_luma_grid(cr), matrix, full, B)
    return from_rgb16(lookup(table, rgb), out_matrix, out_full, D)


# ------------------------------------------------------------------------------------------------ tables and inputs
def identity_table(n):
    """entry k of an axis is round-half-up(65535 k / (n - 1)); exact when n - 1 divides 65535"""
    ax = (np.arange(n, dtype=np.int64) * 65535 * 2 + (n - 1)) // (2 * (n - 1))
    t = np.empty((n, n, n, 3), np.uint16)
    t[..., 0] = ax[None, None, :]
    t[..., 1] = ax[None, :, None]
    t[..., 2] = ax[:, None, None]
    return t


def random_table(n, seed):
    """uniform random entries, with 0 and 65535 among them"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 65536, (n, n, n, 3)).astype(np.uint16)
    t[0, 0, 0] = (0, 65535, 0)
    t[-1, -1, -1] = (65535, 0, 65535)
    t[0, -1, 0] = (65535, 65535, 65535)
    t[-1, 0, -1] = (0, 0, 0)
    return t


def source(kind, w, h, B, seed=0, n=33):
    """(Y, Cb, Cr) of the display size.  noise: full-range noise (above 8 bit also values above the depth); ramp: a grey ramp, chroma at its midpoint, so the three
    fractions of step 3 are equal everywhere; cells: luma at the values whose R' = G' = B' fall on and next to the cell boundaries of a table of n points, chroma
    at its midpoint with a few samples off it"""
    rng = np.random.default_rng(seed + 1000 * B + w)
    dt = dtype(B)
    if kind == "noise":
        top = 1 << (16 if B > 8 else 8)
        return [np.ascontiguousarray(rng.integers(0, top, s).astype(dt)) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    mid, peak = 1 << (B - 1), (1 << B) - 1
    c = np.full((h // 2, w // 2), mid, dt)
    if kind == "ramp":
        y = (np.arange(w * h, dtype=np.int64) * peak // (w * h - 1)).reshape(h, w).astype(dt)
        return [y, c, c.copy()]
    assert kind == "cells"
    bounds = np.arange(n, dtype=np.int64) * 65535 // (n - 1)                      # v at the grid points (rounded down)
    lo, span = 16 << (B - 8), 219 << (B - 8)
    ys = np.clip((bounds * span + 32767) // 65535 + lo, 0, peak)                  # the limited-range luma nearest to each
    vals = np.concatenate([ys - 1, ys, ys + 1]).clip(0, peak)
    y = vals[rng.integers(0, len(vals), (h, w))].astype(dt)
    cr = c.copy()
    cr[::3, ::5] = mid + 1
    return [y, c, cr]
