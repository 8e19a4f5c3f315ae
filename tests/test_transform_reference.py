"""CPU: K3 (forward transform, dead-zone quantiser, scaling, inverse transform) against a plain integer reference written in numpy
int64 (tests/transform_ref.py) from H.265 8.6 and the formulas residual.h states, at every QP 0..51, both bit depths, intra and inter rounding, every size and
DST-VII, on residuals built to sit at the ends of the arithmetic.  The reference does not use the oracle: its matrix comes from the 33
quarter-wave constants, each entry checked against 64 sqrt(2) cos(pi (2n + 1) k / 64).  test_gpu_parity.py holds the device twin."""
import numpy as np
import pytest

from oracle import oracle as O

from tests.transform_ref import DST4, QUANT_SCALE, dct32, matrix, reference  # noqa: F401  (the reference itself: tests/transform_ref.py)


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
