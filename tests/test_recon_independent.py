"""CPU: the samples of every coded stream rebuilt by tests/hevc_recon.py, a reconstruction written from H.265 over the independent syntax reader
(tests/hevc_syntax.py), must equal the oracle pipeline's reconstruction, the repository decoder's output and the stream's decoded picture hash.
The kernels, the oracle and the repository decoder share one author's reading of the sample processes; a rule all three read the same wrong way
would pass every parity test and fail here.

First the reconstruction's stages are pinned by answers worked out by hand: the closed forms of tests/test_oracle_kat.py and
tests/test_decoder_second_opinion.py restated against them, and the edges where a reading most easily goes wrong."""
import collections
import functools

import numpy as np
import pytest

from tests import hevc_recon as R
from tests.test_syntax_independent import CASES, encoded, parsed


def refs(n, left, corner, top):
    """the 4N+1 reference samples from left[y] = p[-1][y] and top[x] = p[x][-1] (2N each)"""
    return np.array(list(reversed(left)) + [corner] + list(top), np.int64)


# ================================================================ 8.6 scaling and transformation
def test_transform_matrix_rows_and_dc():
    m = R.DCT32
    assert list(m[0]) == [64] * 32
    assert list(m[1][:16]) == [90, 90, 88, 85, 82, 78, 73, 67, 61, 54, 46, 38, 31, 22, 13, 4]
    assert list(m[2][:8]) == [90, 87, 80, 70, 57, 43, 25, 9] and list(m[4][:4]) == [89, 75, 50, 18]
    assert list(m[8][:4]) == [83, 36, -36, -83] and list(m[16][:4]) == [64, -64, -64, 64] and list(m[24][:4]) == [36, -83, 83, -36]
    assert list(m[31][:4]) == [4, -13, 22, -31] and list(m[1][16:]) == [-4, -13, -22, -31, -38, -46, -54, -61, -67, -73, -78, -82, -85, -88, -90, -90]
    # a DC-only block is flat: ((64 dc + 64) >> 7) * 64 + (1 << 11)) >> 12 at 8 bit
    for n in (4, 8, 16, 32):
        d = np.zeros((n, n), np.int64)
        d[0, 0] = 1000
        g = (64 * 1000 + 64) >> 7
        assert (R.inverse_transform(d, 8) == (64 * g + 2048) >> 12).all()
    # DST-VII of a DC level: column 0 of the matrix, then row-wise: r[y][x] = ((29 * ((29 d + 64) >> 7)) + ...) by (8-314)
    d = np.zeros((4, 4), np.int64)
    d[0, 0] = 256
    e = [(c * 256 + 64) >> 7 for c in (29, 55, 74, 84)]
    want = [[(e[y] * c + 2048) >> 12 for c in (29, 55, 74, 84)] for y in range(4)]
    assert R.inverse_transform(d, 8, dst=True).tolist() == want


def test_scaling_by_hand_and_the_clips():
    lv = np.zeros((8, 8), np.int64)
    lv[0, 0] = 7
    assert R.scale(lv, 22, 8, 3)[0, 0] == ((7 * 16 * 64 << 3) + 32) >> 6           # levelScale[4] = 64, bdShift 8 + 3 - 5 = 6
    assert R.scale(lv, 22 + 12, 10, 3)[0, 0] == ((7 * 16 * 64 << 5) + 128) >> 8    # 10 bit: Qp'Y = 34, bdShift 8
    lv[0, 0] = 32767
    assert R.scale(lv, 51, 8, 3)[0, 0] == 32767 and R.scale(-lv, 51, 8, 3)[0, 0] == -32768
    # the intermediate clip: a first column of 32767 gives e[0][0] = (64 + 83 + 64 + 36) * 32767, whose (e + 64) >> 7 passes coeffMax
    d = np.zeros((4, 4), np.int64)
    d[:, 0] = 32767
    out = R.inverse_transform(d, 8)
    assert (out[0] == (64 * 32767 + 2048) >> 12).all()                               # g clipped to 32767 before the second stage
    assert [R.qpc_from_qpi(q) for q in range(28, 46)] == [28, 29, 29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37, 38, 39]
    assert R.qpc_from_qpi(51) == 45 and R.qpc_from_qpi(10) == 10 and R.qpc_from_qpi(-12) == -12


# ================================================================ 8.4.4.2 intra
def test_intra_dc_planar_vertical_horizontal_by_hand():
    n = 8
    ref = refs(n, [100] * 16, 80, [60] * 16)
    dc = R.predict_intra(ref, n, 1, 0, 8)
    assert dc[4, 4] == 80 and dc[0, 0] == (100 + 160 + 60 + 2) >> 2 and dc[0, 3] == (60 + 240 + 2) >> 2 and dc[3, 0] == (100 + 240 + 2) >> 2
    assert (R.predict_intra(ref, n, 1, 1, 8) == 80).all()                         # chroma: no DC edge filter
    v = R.predict_intra(ref, n, 26, 0, 8)
    assert (v[:, 1:] == 60).all() and (v[:, 0] == 70).all()                         # 60 + ((100 - 80) >> 1)
    h = R.predict_intra(ref, n, 10, 0, 8)
    assert (h[1:, :] == 100).all() and (h[0, :] == 90).all()                        # 100 + ((60 - 80) >> 1)
    p = R.predict_intra(ref, n, 0, 0, 8)
    assert p[0, 0] == (700 + 60 + 420 + 100 + 8) >> 4 and p[7, 7] == (480 + 800 + 8) >> 4
    # no edge filter at 32x32
    ref32 = refs(32, [100] * 64, 80, [60] * 64)
    assert (R.predict_intra(ref32, 32, 26, 0, 8) == 60).all() and (R.predict_intra(ref32, 32, 1, 0, 8) == 80).all()


@pytest.mark.parametrize("n", [4, 8, 16])
def test_diagonal_modes_are_pure_copies(n):
    ref = np.arange(4 * n + 1) * 3 + 7
    left = lambda y: int(ref[2 * n - 1 - y])        # noqa: E731
    top = lambda x: int(ref[2 * n + 1 + x])         # noqa: E731
    m34, m2, m18 = (R.predict_intra(ref, n, m, 1, 8) for m in (34, 2, 18))
    for y in range(n):
        for x in range(n):
            assert m34[y, x] == top(x + y + 1) and m2[y, x] == left(x + y + 1)
            assert m18[y, x] == (top(x - y - 1) if x > y else left(y - x - 1) if y > x else int(ref[2 * n]))


def test_negative_angle_with_inverse_angle_projection_by_hand():
    """mode 13 (intraPredAngle -9, invAngle -910), 8x8: ref[-1], ref[-2], ref[-3] come from the top row at -1 + ((x * -910 + 128) >> 8) = 3, 6, 10"""
    n = 8
    ref = np.random.default_rng(13).integers(0, 256, 4 * n + 1)
    left = lambda y: int(ref[2 * n - 1 - y])        # noqa: E731
    top = lambda x: int(ref[2 * n + 1 + x])         # noqa: E731
    r = {x: left(x - 1) for x in range(0, n + 1)}
    r[-1], r[-2], r[-3] = top(3), top(6), top(10)
    idx, fact = [-1, -1, -1, -2, -2, -2, -2, -3], [23, 14, 5, 28, 19, 10, 1, 24]
    got = R.predict_intra(ref, n, 13, 1, 8)
    for j in range(n):
        for i in range(n):
            assert got[i, j] == ((32 - fact[j]) * r[i + idx[j] + 1] + fact[j] * r[i + idx[j] + 2] + 16) >> 5, (i, j)
    got = R.predict_intra(ref, n, 11, 1, 8)                                         # (8 * -2) >> 5 = -1: no projection
    for j in range(n):
        for i in range(n):
            assert got[i, j] == (2 * (j + 1) * left(i - 1) + (32 - 2 * (j + 1)) * left(i) + 16) >> 5


def test_reference_filter_rules():
    n = 8
    ref = np.arange(33, dtype=np.int64) * 4
    ref[10] += 40
    for mode, on in ((1, False), (2, True), (18, True), (20, False), (26, False), (10, False), (0, True), (34, True)):
        assert (not np.array_equal(R.filter_refs(ref, n, mode, 8, 1), ref)) == on, mode
    out = R.filter_refs(ref, n, 2, 8, 1)
    assert out[0] == ref[0] and out[32] == ref[32] and out[10] == (ref[9] + 2 * ref[10] + ref[11] + 2) >> 2
    assert np.array_equal(R.filter_refs(np.arange(17), 4, 2, 8, 1), np.arange(17))   # 4x4: never
    # 16x16: |mode - 26| and |mode - 10| must both exceed 1
    r16 = np.arange(65, dtype=np.int64) * 3
    r16[7] += 30
    assert [m for m in range(35) if not np.array_equal(R.filter_refs(r16, 16, m, 8, 1), r16)] == [0] + [m for m in range(2, 35) if m not in (1, 9, 10, 11, 25, 26, 27)]
    # 32x32 flat-ish: bi-linear
    r32 = np.full(129, 100, np.int64)
    r32[0], r32[128] = 96, 104
    o = R.filter_refs(r32, 32, 0, 8, 1)
    assert o[0] == 96 and o[64] == 100 and o[128] == 104 and o[32] == (32 * 100 + 32 * 96 + 32) >> 6


def test_strong_smoothing_threshold_at_10_bit_on_both_sides():
    """1 << (BitDepthY - 5): 32 at 10 bit, 8 at 8 bit.  A top row that bends by one less is smoothed bi-linearly (8-30..8-34), one that bends by
    the threshold gets [1 2 1]; the same for the left column"""
    for bd, thr in ((10, 32), (8, 8)):
        base = 100 << (bd - 8)
        for bend, bilinear in ((thr - 1, True), (thr, False)):
            ramp = [base] * 32 + [base + bend * (k + 1) // 32 for k in range(32)]    # p[31][-1] = base, p[63][-1] = base + bend
            want = [((63 - k) * base + (k + 1) * (base + bend) + 32) >> 6 for k in range(63)]
            out = R.filter_refs(refs(32, [base] * 64, base, ramp), 32, 0, bd, 1)
            assert (list(out[65:128]) == want) == bilinear, (bd, bend)
            if not bilinear:
                assert out[100] == (ramp[34] + 2 * ramp[35] + ramp[36] + 2) >> 2
            out = R.filter_refs(refs(32, ramp, base, [base] * 64), 32, 0, bd, 1)    # pF[-1][y] sits at index 63 - y
            assert ([int(out[63 - k]) for k in range(63)] == want) == bilinear, (bd, bend)
    ref = refs(32, [400] * 32 + [432] * 32, 400, [400] * 64)                          # the left column bends by 32: [1 2 1]
    assert R.filter_refs(ref, 32, 0, 10, 1)[31] == (432 + 2 * 432 + 400 + 2) >> 2
    assert R.filter_refs(ref, 32, 0, 10, 0)[31] == (432 + 2 * 432 + 400 + 2) >> 2   # strong_intra_smoothing_enabled_flag 0: [1 2 1] always


def test_substitution():
    p = np.arange(17, dtype=np.int64) + 50
    assert (R.substitute(p, np.zeros(17, bool), 8) == 128).all() and (R.substitute(p, np.zeros(17, bool), 10) == 512).all()
    avail = np.zeros(17, bool)
    avail[5:9] = True                                                               # only p[-1][3..0]
    out = R.substitute(p, avail, 8)
    assert (out[:5] == p[5]).all() and (out[5:9] == p[5:9]).all() and (out[9:] == p[8]).all()
    avail[:] = True
    avail[12] = False
    out = R.substitute(p, avail, 8)
    assert out[12] == p[11] and (np.delete(out, 12) == np.delete(p, 12)).all()


# ================================================================ 8.5.3.3 inter
def test_interpolation_by_hand():
    flat = np.full((16, 16), 77)
    for mv in [(0, 0), (1, 0), (2, 3), (3, 1), (-5, 7)]:
        assert (R.weighted_default([R.mc_luma(flat, 4, 4, 8, mv, 8)], 8) == 77).all()
        assert (R.weighted_default([R.mc_chroma(flat, 2, 2, 4, mv, 8)], 8) == 77).all()
    ramp = np.tile(np.arange(32) * 8, (32, 1))
    assert (R.weighted_default([R.mc_luma(ramp, 8, 8, 8, (2, 0), 8)], 8)[0] == np.arange(8, 16) * 8 + 4).all()
    assert (R.weighted_default([R.mc_luma(ramp, 8, 8, 8, (1, 0), 8)], 8)[0] == np.arange(8, 16) * 8 + 2).all()
    img = np.random.default_rng(0).integers(0, 256, (32, 32))
    assert np.array_equal(R.weighted_default([R.mc_luma(img, 8, 8, 8, (12, -8), 8)], 8), img[6:14, 11:19])
    taps = [-1, 4, -11, 40, 40, -11, 4, -1]
    x, y = 12, 10
    e = sum(t * int(img[y, x + k - 3]) for k, t in enumerate(taps))
    assert R.mc_luma(img, x, y, 1, (2, 0), 8)[0, 0] == e and R.weighted_default([np.array([[e]])], 8)[0, 0] == min(255, max(0, (e + 32) >> 6))
    col = [sum(t * int(img[y + r, x + k - 3]) for k, t in enumerate(taps)) for r in range(-3, 5)]
    assert R.mc_luma(img, x, y, 1, (2, 2), 8)[0, 0] == sum(t * c for t, c in zip(taps, col)) >> 6
    img10 = img * 4
    e10 = sum(t * int(img10[y, x + k - 3]) for k, t in enumerate(taps)) >> 2       # shift1 = BitDepth - 8 = 2
    assert R.mc_luma(img10, x, y, 1, (2, 0), 10)[0, 0] == e10
    # chroma eighth sample 3: fC = -6 46 28 -4
    cx = sum(t * int(img[5, 7 + k - 1]) for k, t in enumerate((-6, 46, 28, -4)))
    assert R.mc_chroma(img, 7, 5, 1, (3, 0), 8)[0, 0] == cx


def test_motion_vector_40_samples_past_each_corner():
    """every reference sample position is clamped into the coded picture, so a block 40 samples past a corner copies the corner sample; at a
    fractional position as well (the taps sum to 64)"""
    img = np.random.default_rng(3).integers(0, 256, (24, 40))
    h, w = img.shape
    for (x0, y0), mv, corner in (((8, 8), (-4 * 56 + 1, -4 * 56 + 3), img[0, 0]), ((16, 8), (4 * (w + 40 - 16), 4 * (h + 40 - 8) + 2), img[-1, -1]),
                                 ((0, 16), (4 * (w + 40) + 3, -4 * 60), img[0, -1]), ((24, 0), (-4 * 64, 4 * 64 + 1), img[-1, 0])):
        out = R.weighted_default([R.mc_luma(img, x0, y0, 8, mv, 8)], 8)
        assert (out == corner).all(), (x0, y0, mv)
        c = R.weighted_default([R.mc_chroma(img, x0 // 2, y0 // 2, 4, mv, 8)], 8)
        assert (c == corner).all(), (x0, y0, mv)
    # half outside: the rows above the picture repeat row 0
    got = R.mc_luma(img, 8, 0, 8, (0, -4 * 5), 8) >> 6
    assert np.array_equal(got, np.vstack([np.repeat(img[:1, 8:16], 5, 0), img[0:3, 8:16]]))


def test_ten_bit_bi_prediction_rounding():
    """(8-262) shift2 = 15 - 10 = 5, offset2 = 16: 16008 + 16008 -> (32016 + 16) >> 5 = 1001 (1000 without the offset); uni (8-252)
    shift1 = 4, offset1 = 8: 16008 -> 1001"""
    a = np.array([[16008, 16007, 0, 16383 * 1]])
    b = np.array([[16008, 16008, 0, 16383]])
    assert R.weighted_default([a, b], 10).tolist() == [[1001, 1000, 0, 1023]]
    assert R.weighted_default([a], 10).tolist() == [[1001, 1000, 0, 1023]]
    assert R.weighted_default([np.array([[-100]]), np.array([[-100]])], 10).tolist() == [[0]]
    # 8 bit: shift2 = 7, offset 64
    assert R.weighted_default([np.array([[8000]]), np.array([[8064]])], 8).tolist() == [[(16064 + 64) >> 7]]


# ================================================================ 8.7.2 deblocking
def grid(w, h, log2, intra=True, qp=37, mvx=None):
    """a one-slice picture of square CUs of 1 << log2; inter CUs predict from picture 0 with vector (mvx[cu column], 0)"""
    g = R.Grid(h // 4, w // 4)
    yy, xx = np.mgrid[0:h // 4, 0:w // 4]
    g.cuid = (yy >> (log2 - 2)) * 1000 + (xx >> (log2 - 2))
    g.intra[:] = int(intra)
    g.qp[:] = qp
    if not intra:
        g.pf[0][:], g.poc[0][:] = 1, 0
        if mvx is not None:
            g.mvx[0][:] = np.array(mvx)[xx >> (log2 - 2)]
    return g


def step(w, h, x0, a, b):
    y = np.full((h, w), a, np.int64)
    y[:, x0:] = b
    c = np.full((h // 2, w // 2), a, np.int64)
    c[:, x0 // 2:] = b
    return [y, c, c.copy()]


def test_deblocking_strong_normal_and_chroma_by_hand():
    """bS 2, QP 37: beta' 36, tC' 5.  A step of 10 -> strong; a step of 20 -> normal, delta 8 clipped to tC 5, p1 / q1 by +-(tC >> 1)"""
    pl = step(16, 16, 8, 100, 110)
    R.deblock(pl, grid(16, 16, 3), 8)
    assert pl[0][5, 4:12].tolist() == [100, 101, 103, 104, 106, 108, 109, 110] and (pl[0][:, 4:12] == pl[0][5, 4:12]).all()
    assert (pl[1] == step(16, 16, 8, 100, 110)[1]).all()                            # chroma x = 4 is off the 8-sample chroma grid
    pl = step(16, 16, 8, 100, 120)
    R.deblock(pl, grid(16, 16, 3), 8)
    assert pl[0][9, 4:12].tolist() == [100, 100, 102, 105, 115, 118, 120, 120]
    # 16x16 CUs: the edge x = 16 is on the chroma grid; QpC(37) = 34, tC' = tC'[36] = 4, delta = ((10 << 2) + 100 - 110 + 4) >> 3 = 4
    pl = step(32, 16, 16, 100, 110)
    R.deblock(pl, grid(32, 16, 4), 8)
    assert pl[1][3, 6:10].tolist() == [100, 104, 106, 110] and (pl[2] == pl[1]).all()
    # the large step of test_oracle_kat: QP 30, bS 2 -> tC 3, beta 22; normal, delta 23 clipped to 3, dEp -> p1 moves by 1
    pl = step(32, 32, 8, 60, 100)
    R.deblock(pl, grid(32, 32, 3, qp=30), 8)
    assert pl[0][0, 5:11].tolist() == [60, 61, 63, 97, 99, 100]


def test_chroma_deblocking_skipped_at_bs_1_and_off_the_16_luma_grid():
    f = step(32, 16, 16, 100, 110)
    pl = [a.copy() for a in f]
    R.deblock(pl, grid(32, 16, 4, intra=False, mvx=[0, 4]), 8)                      # inter, vectors 4 quarter samples apart: bS 1
    assert not np.array_equal(pl[0], f[0]) and (pl[1] == f[1]).all() and (pl[2] == f[2]).all()
    pl = [a.copy() for a in f]
    R.deblock(pl, grid(32, 16, 4, intra=False, mvx=[0, 3]), 8)                      # 3 quarter samples: bS 0
    assert all((a == b).all() for a, b in zip(pl, f))
    g = grid(32, 16, 4, intra=False, mvx=[0, 0])
    g.nz[:, 4:] = 1                                                                 # a coded luma TB on one side: bS 1, chroma untouched
    pl = [a.copy() for a in f]
    R.deblock(pl, g, 8)
    assert not np.array_equal(pl[0], f[0]) and (pl[1] == f[1]).all()
    # bS 2 at x = 8 (chroma x = 4) and x = 24 (chroma 12): off the chroma grid; x = 16 filtered
    f = step(32, 16, 8, 100, 110)
    f[1][:, 8:] = 130
    f[1][:, 12:] = 150
    pl = [a.copy() for a in f]
    R.deblock(pl, grid(32, 16, 3), 8)
    assert (pl[1][:, [3, 4, 11, 12]] == f[1][:, [3, 4, 11, 12]]).all() and (pl[1][:, 7:9] != f[1][:, 7:9]).all()
    # two vectors each, same two pictures in swapped lists: compared by picture, not by list -> bS 0
    g = grid(32, 16, 4, intra=False)
    g.pf[1][:], g.poc[1][:] = 1, 8
    g.poc[0][:, 4:], g.poc[1][:, 4:] = 8, 0                                         # q side: list 0 -> picture 8, list 1 -> picture 0
    q, p = (slice(None), slice(2, 8, 2)), (slice(None), slice(1, 7, 2))
    assert (R.motion_bs(g, q, p)[:, 1] == 0).all()
    g.mvy[1][:, 4:] = 4                                                             # the vector of picture 0 on the q side moved by 4
    assert (R.motion_bs(g, q, p)[:, 1] == 1).all()


def test_deblocking_tc_and_beta_scale_with_bit_depth():
    """10 bit: beta = 36 * 4 = 144, tC = 5 * 4 = 20.  A step of 40 -> strong, p0' = 415; a step of 52 -> normal, delta = 20 = tC"""
    pl = step(16, 16, 8, 400, 440)
    R.deblock(pl, grid(16, 16, 3), 10)
    assert pl[0][2, 4:12].tolist() == [400, 405, 410, 415, 425, 430, 435, 440]
    pl = step(16, 16, 8, 400, 452)
    R.deblock(pl, grid(16, 16, 3), 10)
    assert pl[0][2, 6:10].tolist() == [410, 420, 432, 442]
    f = step(16, 16, 8, 400, 440)
    pl = [a.copy() for a in f]
    R.deblock(pl, grid(16, 16, 3, qp=15), 10)
    assert all((a == b).all() for a, b in zip(pl, f))


def test_slice_edge_not_filtered_when_the_lower_slice_says_so():
    f = step(16, 32, 0, 100, 100)
    f[0][16:], f[1][8:], f[2][8:] = 110, 110, 110
    for across, moved in ((1, True), (0, False)):
        g = grid(16, 32, 3)
        g.slice[4:] = 1
        g.across = np.array([1, across])
        g.off, g.beta, g.tc = np.zeros(2, np.int64), np.zeros(2, np.int64), np.zeros(2, np.int64)
        pl = [a.copy() for a in f]
        R.deblock(pl, g, 8)
        assert (not np.array_equal(pl[0], f[0])) == moved


# ================================================================ 8.7.3 SAO
def sao_prm(types, classes, bands, offsets):
    return [{"type": list(types), "eo_class": list(classes), "band_pos": list(bands), "offset": [list(o) for o in offsets]}]


def test_sao_band_and_edge_by_hand():
    y = np.full((32, 32), 64)
    y[10, 10], y[20, 20] = 60, 70
    prm = sao_prm((2, 1), (0, 0), (0, 12, 24), ((3, 1, -1, -2), (5, 0, 0, 0), (0, -6, 0, 0)))
    got = R.sao_plane(y, 0, 8, 5, prm)
    want = y.copy()
    want[10, 10], want[10, 9], want[10, 11] = 63, 63, 63
    want[20, 20], want[20, 19], want[20, 21] = 68, 65, 65
    assert np.array_equal(got, want)
    assert (R.sao_plane(np.full((16, 16), 100), 1, 8, 4, prm) == 105).all() and (R.sao_plane(np.full((16, 16), 200), 2, 8, 4, prm) == 194).all()


def test_sao_band_positions_wrap_round():
    """sao_band_position 30: the four bands are 30, 31, 0, 1 (bandTable[(k + 30) & 31] = k + 1); 10 bit: bandShift 5"""
    prm = sao_prm((1, 1), (0, 0), (30, 0, 0), ((1, 2, 3, 4),) * 3)
    v = np.array([[30 * 8, 31 * 8 + 7, 0, 15, 16, 29 * 8 + 7]])
    assert R.sao_plane(v, 0, 8, 5, prm).tolist() == [[241, 255, 3, 19, 16, 239]]                   # 255 + 2 clipped
    v10 = np.array([[30 * 32, 1023, 0, 63, 64]])
    assert R.sao_plane(v10, 0, 10, 5, prm).tolist() == [[961, 1023, 3, 67, 64]]
    prm = sao_prm((1, 1), (0, 0), (29, 0, 0), ((-7, 7, -7, 7),) * 3)
    assert R.sao_plane(np.array([[29 * 8, 31 * 8, 0, 3]]), 0, 8, 5, prm).tolist() == [[225, 241, 7, 10]]


def test_sao_edge_samples_on_the_picture_border_are_kept():
    """a local minimum on the border has no neighbour on one side: SaoOffsetVal 0 for every class that looks across the border"""
    y = np.full((16, 16), 50)
    y[0, 5], y[5, 0], y[15, 15], y[6, 6] = 40, 40, 40, 40
    for e in range(4):
        out = R.sao_plane(y, 0, 8, 5, sao_prm((2, 0), (e, 0), (0, 0, 0), ((2, 1, -1, -2), (0,) * 4, (0,) * 4)))
        assert out[6, 6] == 42
        assert out[0, 5] == (42 if e == 0 else 40) and out[5, 0] == (42 if e == 1 else 40) and out[15, 15] == 40, e
    # across a slice edge whose later slice forbids it: kept as well
    region = (np.array([0, 1]), np.array([0, 1]), np.array([1, 0]), np.array([0, 0]), 1)
    y = np.full((64, 32), 50)
    y[32, 7] = 40
    out = R.sao_plane(y, 0, 8, 5, sao_prm((2, 0), (1, 0), (0, 0, 0), ((2, 1, -1, -2), (0,) * 4, (0,) * 4)) * 2, region)
    assert out[32, 7] == 40 and out[31, 7] == 50
    region = (np.array([0, 1]), np.array([0, 1]), np.array([1, 1]), np.array([0, 0]), 1)
    out = R.sao_plane(y, 0, 8, 5, sao_prm((2, 0), (1, 0), (0, 0, 0), ((2, 1, -1, -2), (0,) * 4, (0,) * 4)) * 2, region)
    assert out[32, 7] == 42 and out[31, 7] == 49


# ================================================================ every CPU stream
@functools.lru_cache(maxsize=None)
def rebuilt(name):
    stats = {}
    out = R.reconstruct(parsed(name)[1], stats)
    return out, stats


def display_index(st):
    """display position of every picture in decoding order: the IDR's position plus the POC (closed GOPs)"""
    out, base = [], 0
    for i, p in enumerate(st.pictures):
        if p.nal_type in (19, 20):
            base = i
        out.append(base + p.poc)
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_reconstruction_equals_the_oracle_the_decoder_and_the_hash(name):
    from oracle import oracle as O
    _, stream, _, _, recs = encoded(name)
    st = parsed(name)[1]
    out, stats = rebuilt(name)
    assert [p for p, *_ in out] == [p.poc for p in st.pictures]
    if recs is not None:
        assert len(recs) == len(out)
        for k, ((poc, y, u, v), r) in enumerate(zip(out, recs)):
            for c, (a, b) in enumerate(((y, r.y), (u, r.u), (v, r.v))):
                assert a.shape == b.shape and np.array_equal(a, b), \
                    "picture %d (POC %d) plane %d: %d samples differ from the oracle pipeline, first at %s" % (k, poc, c, int((a != b).sum()), np.argwhere(a != b)[:1].tolist())
    frames, _ = O.decode(stream)
    assert len(frames) == len(out)
    for (poc, y, u, v), d in zip(out, display_index(st)):
        f = frames[d]
        assert np.array_equal(y, f.y) and np.array_equal(u, f.u) and np.array_equal(v, f.v), "display picture %d differs from the repository decoder" % d
    for k, hh in enumerate(stats["hash"]):
        if hh is not None:
            assert hh[1] == hh[2], "picture %d: the hash SEI says %s, the reconstruction hashes to %s" % (k, hh[1], hh[2])
    assert (name.startswith("hash-")) == any(hh is not None for hh in stats["hash"])


def test_every_sample_process_branch_is_reached():
    cov = collections.Counter()
    for name in CASES:
        cov.update(rebuilt(name)[1]["cov"])
    missing = []
    for c, sizes in ((0, (4, 8, 16, 32)), (1, (4, 8, 16)), (2, (4, 8, 16))):
        for n in sizes:
            missing += [("intra", c, n, m) for m in range(35) if not cov["intra", c, n, m]]
    missing += [("luma_frac", fx, fy) for fx in range(4) for fy in range(4) if not cov["luma_frac", fx, fy]]
    missing += [k for k in [("inter", "bi"), ("inter", "uni"), ("mc", "outside"), ("deblock", "bs1"), ("deblock", "bs2"), ("deblock", "strong"),
                            ("deblock", "normal"), ("deblock", "chroma"), ("deblock", "slice_edge_unfiltered"), "dst", ("smoothing", "bilinear"),
                            ("smoothing", "threshold_missed"), ("smoothing", "121")] if not cov[k]]
    for c in range(3):
        missing += [k for k in [("sao_band", c), ("sao_band_wrap", c), ("sao_edge_kept", c)] + [("sao_edge", c, e) for e in range(4)] if not cov[k]]
    assert not missing, missing
