"""CPU: K3 (forward transform, dead-zone quantiser, scaling, inverse transform) against a plain integer reference written here in numpy
int64 from H.265 8.6 and the formulas residual.h states, at every QP 0..51, both bit depths, intra and inter rounding, every size and
DST-VII, on residuals built to sit at the ends of the arithmetic.  The reference does not use the oracle: its matrix comes from the 33
quarter-wave constants, each entry checked against 64 sqrt(2) cos(pi (2n + 1) k / 64).  test_gpu_parity.py holds the device twin."""
import numpy as np
import pytest

from oracle import oracle as O

# 64 sqrt(2) cos(pi m / 64) rounded to the HEVC integers, m = 0..32 (m = 0: the DC row, scaled by 1 / sqrt(2) to 64)
QUARTER_WAVE = (64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4, 0)
DST4 = ((29, 55, 74, 84), (74, 74, 0, -74), (84, -29, -74, 55), (55, -84, 74, -29))
LEVEL_SCALE = (40, 45, 51, 57, 64, 72)                                 # 8.6.4.1 levelScale[]
QUANT_SCALE = tuple(int(round((1 << 20) / s)) for s in LEVEL_SCALE)    # the encoder's inverse of it: 26214, 23302, 20560, 18396, 16384, 14564
I16 = (-32768, 32767)


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


def reference(res, log2n, qp, bit_depth, intra, dst=False):
    """res: (blocks, n, n) residuals -> (levels, reconstructed residuals), both (blocks, n, n) int64.  Forward: rows, shift log2n + bd - 9
    (16-bit intermediate, checked), columns, shift log2n + 6, clip to 16 bit.  Quantiser: qP = qp + 6 (bd - 8), qbits = 14 + qP / 6 +
    (15 - bd - log2n), offset 171 (intra) / 85 (inter) << (qbits - 9), magnitude at most 32767.  Scaling (8.6.4.1, m = 16): bdShift =
    bd + log2n - 5, clip to 16 bit.  Inverse (8.6.4.2): columns, (x + 64) >> 7, clip to 16 bit; rows, shift 20 - bd (16-bit, checked).
    A block without a non-zero level reconstructs to zero."""
    t = matrix(log2n, dst)
    r = np.asarray(res, np.int64)
    tmp = _round_shift(np.einsum("bxy,uy->bxu", r, t), log2n + bit_depth - 9)      # tmp[y][u] = sum_x r[y][x] T[u][x]
    _fits16(tmp, "forward stage 1")
    coef = np.clip(_round_shift(np.einsum("vy,byu->bvu", t, tmp), log2n + 6), *I16)
    q = qp + 6 * (bit_depth - 8)
    qbits = 14 + q // 6 + (15 - bit_depth - log2n)
    add = (171 if intra else 85) << (qbits - 9)
    mag = np.minimum((np.abs(coef) * QUANT_SCALE[q % 6] + add) >> qbits, 32767)
    lvl = np.where(coef < 0, -mag, mag)
    bd_shift = bit_depth + log2n - 5
    deq = np.clip((lvl * 16 * LEVEL_SCALE[q % 6] << (q // 6)) + (1 << (bd_shift - 1)) >> bd_shift, *I16)
    g = np.clip((np.einsum("jy,bjx->byx", t, deq) + 64) >> 7, *I16)                  # columns: g[y][x] = sum_j T[j][y] d[j][x]
    rec = _round_shift(np.einsum("byj,jx->byx", g, t), 20 - bit_depth)               # rows: r[y][x] = sum_j g[y][j] T[j][x]
    _fits16(rec, "inverse stage 2")
    rec[~lvl.any(axis=(1, 2))] = 0
    return lvl, rec


def adversarial_residuals(log2n, bit_depth, dst=False, seed=0):
    """residuals at the ends of the transform's range: +-amp DC, the sign patterns of basis products T_k x T_l, +-amp checkerboards,
    +-amp impulses in each corner, random +-amp per sample (amp = 2^bd - 1)"""
    n, amp = 1 << log2n, (1 << bit_depth) - 1
    t = matrix(log2n, dst)
    rng = np.random.default_rng(seed + 97 * log2n + bit_depth + 5 * dst)
    out = [np.zeros((n, n)), np.full((n, n), amp), np.full((n, n), -amp)]
    ks = range(n) if n <= 8 else sorted({0, 1, 2, 3, n // 2 - 1, n // 2, n - 2, n - 1} | set(rng.integers(0, n, 4).tolist()))
    for k in ks:
        for l in ks:
            s = np.sign(np.outer(t[k], t[l]))
            s[s == 0] = 1
            out.append(amp * s if (k + l) % 2 == 0 else -amp * s)
    yy, xx = np.mgrid[0:n, 0:n]
    chk = np.where((xx + yy) % 2 == 0, amp, -amp)
    out += [chk, -chk]
    for cy in (0, n - 1):
        for cx in (0, n - 1):
            for s in (amp, -amp):
                b = np.zeros((n, n), np.int64)
                b[cy, cx] = s
                out.append(b)
    out += [amp * (2 * rng.integers(0, 2, (n, n)) - 1) for _ in range(4)]
    return np.stack(out).astype(np.int64)


def dead_zone_residuals(log2n, qp, bit_depth, intra):
    """small flat residuals around the one where the DC level turns from 0 to 1 at this QP (the DC coefficient of a flat residual v is
    v * 2^(15 - bd)), plus the same with a +-1 ripple"""
    n = 1 << log2n
    q = qp + 6 * (bit_depth - 8)
    qbits = 14 + q // 6 + (15 - bit_depth - log2n)
    add = (171 if intra else 85) << (qbits - 9)
    v = ((1 << qbits) - add) / QUANT_SCALE[q % 6] / (1 << (15 - bit_depth))
    vals = sorted({max(1, int(v) + d) for d in (-1, 0, 1, 2)})
    ripple = np.where((np.mgrid[0:n, 0:n].sum(0)) % 2 == 0, 1, -1)
    out = [np.full((n, n), s * x) for x in vals for s in (1, -1)] + [x * np.ones((n, n), np.int64) + ripple for x in vals]
    return np.stack(out).astype(np.int64)


SIZES = [(2, 0), (2, 1), (3, 0), (4, 0), (5, 0)]


def test_matrix_entries_follow_the_cosines():
    m = dct32()
    k, n = np.mgrid[0:32, 0:32]
    ideal = 64 * np.sqrt(2) * np.cos(np.pi * (2 * n + 1) * k / 64)
    ideal[0] = 64
    assert np.abs(m - ideal).max() <= 2
    assert (m[0] == 64).all() and [m[k, 0] for k in (1, 2, 4, 8, 16)] == [90, 90, 89, 83, 64]
    d = np.array(DST4)
    i, j = np.mgrid[0:4, 0:4]
    assert np.abs(d - 128 * 2 / 3 * np.sin(np.pi * (2 * i + 1) * (j + 1) / 9)).max() <= 2
    for log2n in (2, 3, 4, 5):          # the smaller matrices are sections of the 32-point one; rows orthogonal up to the integer rounding
        t = matrix(log2n)
        g = t @ t.T
        assert np.abs(g - np.diag(np.diag(g))).max() <= 0.003 * 4096 * (1 << log2n)
        assert np.abs(np.diag(g) - 4096 * (1 << log2n)).max() <= 0.003 * 4096 * (1 << log2n)
    assert np.array_equal(O.transform_matrix().astype(np.int64), dct32())


def test_reference_reaches_the_ends_of_its_range():
    """the adversarial blocks must drive the arithmetic to where it can go wrong: a QP 0 level >= 4000 (long coeff_abs_level_remaining
    escapes), the scaling clip at QP 51 (intra 32x32 at full amplitude), DC levels on both sides of the dead zone"""
    res = adversarial_residuals(5, 8)
    lv0, _ = reference(res, 5, 0, 8, True)
    assert np.abs(lv0).max() >= 4000
    lv51, _ = reference(res, 5, 51, 8, True)
    assert (np.abs(lv51) >= 36).any()       # 36 x 16 x 57 << 8 >> 8 = 32832: the 16-bit scaling clip binds
    for intra in (0, 1):
        for qp in (30, 37, 51):           # (below ~QP 26 a flat residual of 1 already codes a level)
            lv, _ = reference(dead_zone_residuals(3, qp, 8, intra), 3, qp, 8, intra)
            dc = np.abs(lv[:, 0, 0])
            assert (dc == 0).any() and (dc >= 1).any(), (qp, intra)


@pytest.mark.parametrize("log2n,dst", SIZES)
@pytest.mark.parametrize("bd", [8, 10])
def test_oracle_transform_quant_equals_the_integer_reference_at_every_qp(log2n, dst, bd):
    n = 1 << log2n
    rng = np.random.default_rng(11 * log2n + bd + dst)
    amp = (1 << bd) - 1
    base = np.concatenate([adversarial_residuals(log2n, bd, dst), rng.integers(-amp, amp + 1, (6, n, n))])
    if n == 32:
        base = base[::2]                    # the oracle is called block by block: every other 32x32 pattern keeps this test short
    coefs = {}
    for qp in range(52):
        for intra in (1, 0):
            res = np.concatenate([base, dead_zone_residuals(log2n, qp, bd, intra)])
            want_l, want_r = reference(res, log2n, qp, bd, intra, dst)
            for b in range(len(res)):
                key = res[b].tobytes()
                if key not in coefs:
                    coefs[key] = O.fwd_transform(res[b].astype(np.int16), dst=bool(dst), bit_depth=bd)
                lv = O.quant(coefs[key], qp, bit_depth=bd, intra=bool(intra))
                assert np.array_equal(lv, want_l[b]), (qp, intra, b)
                rc = O.inv_transform(O.dequant(lv, qp, bit_depth=bd), dst=bool(dst), bit_depth=bd) if lv.any() else np.zeros_like(lv)
                assert np.array_equal(rc, want_r[b]), (qp, intra, b)
