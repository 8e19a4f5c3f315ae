"""K3 (forward transform, dead-zone quantiser, scaling, inverse transform) as a plain integer reference in numpy int64, written from H.265 8.6 and the
formulas hevc_amd/csrc/kernels/residual.h states.  Its matrix comes from the 33 quarter-wave constants.  tests/test_transform_reference.py holds the
oracle to it (and checks the matrix against the cosines), tests/test_gpu_parity.py the device; tests/hevc_intra_plan.py prices residuals with it.

Imports: numpy and the standard library only (tests/test_syntax_independent.py checks it)."""
import functools

import numpy as np

# 64 sqrt(2) cos(pi m / 64) rounded to the HEVC integers, m = 0..32 (m = 0: the DC row, scaled by 1 / sqrt(2) to 64)
QUARTER_WAVE = (64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4, 0)
DST4 = ((29, 55, 74, 84), (74, 74, 0, -74), (84, -29, -74, 55), (55, -84, 74, -29))
LEVEL_SCALE = (40, 45, 51, 57, 64, 72)                                 # 8.6.4.1 levelScale[]
QUANT_SCALE = tuple(int(round((1 << 20) / s)) for s in LEVEL_SCALE)    # the encoder's inverse of it: 26214, 23302, 20560, 18396, 16384, 14564
I16 = (-32768, 32767)


@functools.lru_cache(maxsize=None)                     # one array for every caller, so it is read-only: matrix() hands out views of it
def dct32() -> np.ndarray:
    m = np.empty((32, 32), np.int64)
    for k in range(32):
        for n in range(32):
            if k == 0:
                m[k, n] = QUARTER_WAVE[0]
                continue
            a = (2 * n + 1) * k % 128                  # cos(pi a / 64): fold into the first quarter wave
            a = 128 - a if a > 64 else a
            m[k, n] = QUARTER_WAVE[a] if a <= 32 else -QUARTER_WAVE[64 - a]
    m.setflags(write=False)
    return m


def matrix(log2n, dst=False) -> np.ndarray:
    """8.6.4.2: the nTbS-point matrix is every (32 / nTbS)-th row of the 32-point one, first nTbS columns; DST-VII for 4x4 luma intra"""
    if dst:
        return np.array(DST4, np.int64)
    n = 1 << log2n
    return dct32()[::32 // n, :n]


def _round_shift(x, sh):
    return (x + (1 << (sh - 1))) >> sh if sh > 0 else x


def _fits16(x, what):
    assert x.min() >= I16[0] and x.max() <= I16[1], f"{what} leaves 16 bits: {x.min()}..{x.max()}"


def forward(res, log2n, bit_depth, dst=False):
    """res: (blocks, n, n) residuals -> coefficients.  Rows, shift log2n + bd - 9 (16-bit intermediate, checked), columns, shift log2n + 6, clip to 16 bit"""
    t = matrix(log2n, dst)
    r = np.asarray(res, np.int64)
    tmp = _round_shift(np.einsum("bxy,uy->bxu", r, t), log2n + bit_depth - 9)      # tmp[y][u] = sum_x r[y][x] T[u][x]
    _fits16(tmp, "forward stage 1")
    return np.clip(_round_shift(np.einsum("vy,byu->bvu", t, tmp), log2n + 6), *I16)


def quantise(coef, log2n, qp, bit_depth, intra):
    """coefficients -> levels: qP = qp + 6 (bd - 8), qbits = 14 + qP / 6 + (15 - bd - log2n), offset 171 (intra) / 85 (inter) << (qbits - 9),
    magnitude at most 32767"""
    q = qp + 6 * (bit_depth - 8)
    qbits = 14 + q // 6 + (15 - bit_depth - log2n)
    add = (171 if intra else 85) << (qbits - 9)
    mag = np.minimum((np.abs(coef) * QUANT_SCALE[q % 6] + add) >> qbits, 32767)
    return np.where(coef < 0, -mag, mag)


def scale(lvl, log2n, qp, bit_depth):
    """levels -> scaled levels (8.6.4.1, m = 16): bdShift = bd + log2n - 5, clip to 16 bit"""
    q = qp + 6 * (bit_depth - 8)
    bd_shift = bit_depth + log2n - 5
    return np.clip((np.asarray(lvl, np.int64) * 16 * LEVEL_SCALE[q % 6] << (q // 6)) + (1 << (bd_shift - 1)) >> bd_shift, *I16)


def inverse(deq, log2n, bit_depth, dst=False):
    """scaled levels -> residuals (8.6.4.2): columns, (x + 64) >> 7, clip to 16 bit; rows, shift 20 - bd (16-bit, checked)"""
    t = matrix(log2n, dst)
    g = np.clip((np.einsum("jy,bjx->byx", t, deq) + 64) >> 7, *I16)                  # columns: g[y][x] = sum_j T[j][y] d[j][x]
    rec = _round_shift(np.einsum("byj,jx->byx", g, t), 20 - bit_depth)               # rows: r[y][x] = sum_j g[y][j] T[j][x]
    _fits16(rec, "inverse stage 2")
    return rec


def reference(res, log2n, qp, bit_depth, intra, dst=False):
    """res: (blocks, n, n) residuals -> (levels, reconstructed residuals), both (blocks, n, n) int64: forward, quantise, scale, inverse (above).
    A block without a non-zero level reconstructs to zero."""
    lvl = quantise(forward(res, log2n, bit_depth, dst), log2n, qp, bit_depth, intra)
    rec = inverse(scale(lvl, log2n, qp, bit_depth), log2n, bit_depth, dst)
    rec[~lvl.any(axis=(1, 2))] = 0
    return lvl, rec
