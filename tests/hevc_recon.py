"""Sample reconstruction of the streams tests/hevc_syntax.py reads -- TEST INFRASTRUCTURE, NOT PRODUCT.

A third witness for sample values, beside the HIP kernels and the oracle (oracle/hevc_oracle.c, oracle/hevc_dec*.c): written clause by clause from
ITU-T H.265 (v1, 04/2013) over the output of the independent syntax reader, never from this repository's kernels, oracle or decoder.  It imports
only the standard library, numpy, tests.hevc_syntax and tests.pichash_ref (tests/test_syntax_independent.py checks that), and its tables are its
own transcription of the standard.

The subset is the encoder's: CTB 32, CU 8..32, TU = CU except intra NxN (four 4x4 luma TBs and one 4x4 TB per chroma component at the 8x8 CU),
2Nx2N inter with one picture per list, QpY = SliceQpY (no cu_qp_delta), no scaling lists.

reconstruct(stream) -> [(poc, y, u, v)] in decoding order, uint16 planes at the coded size.  With stats={} it also leaves there the pictures
before deblocking ("pre"), after deblocking ("dbk"), the decoded picture hash check ("hash": per picture None or (hash_type, the SEI's values,
the values of the reconstruction)) and a Counter of the sample-process branches that were taken ("cov").
"""
from __future__ import annotations

import collections

import numpy as np

from tests import hevc_syntax as S
from tests import pichash_ref as H

# ================================================================ tables
# 8.6.4.2 transMatrix (32x32): row k holds the integers the standard lists for cos((2n + 1) k pi / 64).  Each entry is, up to its sign, one of the
# magnitudes below, indexed by the angle a = (2n + 1) k mod 128 folded into 0..32 (the values of the standard's columns 0 of rows 0..31).
_COS = {0: 64, 16: 64, 8: 83, 24: 36, 4: 89, 12: 75, 20: 50, 28: 18, 2: 90, 6: 87, 10: 80, 14: 70, 18: 57, 22: 43, 26: 25, 30: 9,
        1: 90, 3: 90, 5: 88, 7: 85, 9: 82, 11: 78, 13: 73, 15: 67, 17: 61, 19: 54, 21: 46, 23: 38, 25: 31, 27: 22, 29: 13, 31: 4, 32: 0}


def _dct32():
    m = np.zeros((32, 32), np.int64)
    for k in range(32):
        for n in range(32):
            a = ((2 * n + 1) * k) % 128
            if a > 64:
                a = 128 - a                                     # cos(2 pi - t) = cos t
            s = 1
            if a > 32:
                a, s = 64 - a, -1                               # cos(pi - t) = -cos t
            m[k, n] = s * _COS[a]
    return m


DCT32 = _dct32()
DST4 = np.array([[29, 55, 74, 84], [74, 74, 0, -74], [84, -29, -74, 55], [55, -84, 74, -29]], np.int64)     # 8.6.4.2, trType 1
LEVEL_SCALE = (40, 45, 51, 57, 64, 72)                          # 8.6.3 levelScale[]
QPC_TABLE = {30: 29, 31: 30, 32: 31, 33: 32, 34: 33, 35: 33, 36: 34, 37: 34, 38: 35, 39: 35, 40: 36, 41: 36, 42: 37, 43: 37}   # Table 8-10

# Table 8-4 intraPredAngle (modes 2..34) and Table 8-5 invAngle (modes 11..25)
INTRA_ANGLE = dict(zip(range(2, 35), (32, 26, 21, 17, 13, 9, 5, 2, 0, -2, -5, -9, -13, -17, -21, -26, -32,
                                      -26, -21, -17, -13, -9, -5, -2, 0, 2, 5, 9, 13, 17, 21, 26, 32)))
INV_ANGLE = dict(zip(range(11, 26), (-4096, -1638, -910, -630, -482, -390, -315, -256, -315, -390, -482, -630, -910, -1638, -4096)))
HOR_VER_DIST_THRES = {8: 7, 16: 1, 32: 0}                       # 8.4.4.2.3 intraHorVerDistThres[nTbS]

# luma quarter-sample 8-tap fL[xFrac] and chroma eighth-sample 4-tap fC[xFrac] (8.5.3.3.3.1, 8.5.3.3.3.2)
FL = np.array([[0, 0, 0, 64, 0, 0, 0, 0], [-1, 4, -10, 58, 17, -5, 1, 0], [-1, 4, -11, 40, 40, -11, 4, -1], [0, 1, -5, 17, 58, -10, 4, -1]], np.int64)
FC = np.array([[0, 64, 0, 0], [-2, 58, 10, -2], [-4, 54, 16, -2], [-6, 46, 28, -4], [-4, 36, 36, -4], [-4, 28, 46, -6], [-2, 16, 54, -4],
               [-2, 10, 58, -2]], np.int64)

# 8.7.2.5.3 beta' for Q = 0..51 and tC' for Q = 0..53
BETA_TABLE = np.array([0] * 16 + list(range(6, 19)) + list(range(20, 65, 2)), np.int64)
TC_TABLE = np.array([0] * 18 + [1] * 9 + [2] * 4 + [3] * 4 + [4] * 3 + [5] * 2 + [6] * 2 + [7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24], np.int64)
assert len(BETA_TABLE) == 52 and len(TC_TABLE) == 54


def qpc_from_qpi(qpi):
    """Table 8-10, ChromaArrayType 1"""
    if qpi < 30:
        return qpi
    if qpi > 43:
        return qpi - 6
    return QPC_TABLE[qpi]


# ================================================================ 8.6.2-8.6.4 scaling and transformation
def scale(levels, qp, bd, log2):
    """8.6.3 with m = 16: d = Clip3(coeffMin, coeffMax, ((TransCoeffLevel * m * levelScale[qP % 6] << (qP / 6)) + (1 << (bdShift - 1))) >> bdShift),
    bdShift = BitDepth + Log2(nTbS) - 5; qp is Qp'Y / Qp'Cb / Qp'Cr (QpBdOffset included)"""
    bdshift = bd + log2 - 5
    d = ((np.asarray(levels, np.int64) * 16 * LEVEL_SCALE[qp % 6]) << (qp // 6)) + (1 << (bdshift - 1))
    return np.clip(d >> bdshift, -32768, 32767)


def inverse_transform(d, bd, dst=False):
    """8.6.4.2: every column, then every row, y[i] = sum_j transMatrix[j][i] x[j] (rows j * 32 / nTbS of the 32x32 matrix); the intermediate
    values are Clip3(coeffMin, coeffMax, (e + 64) >> 7), the second stage shifts by bdShift = 20 - BitDepth"""
    n = d.shape[0]
    t = DST4 if dst else DCT32[::32 // n, :n]
    e = t.T @ np.asarray(d, np.int64)
    g = np.clip((e + 64) >> 7, -32768, 32767)
    r = g @ t
    sh = 20 - bd
    return (r + (1 << (sh - 1))) >> sh


def residual(levels, qp, bd, dst=False):
    n = levels.shape[0]
    if not levels.any():
        return np.zeros((n, n), np.int64)
    return inverse_transform(scale(levels, qp, bd, n.bit_length() - 1), bd, dst)


# ================================================================ 8.4.4.2 intra sample prediction
# The 4N + 1 reference samples p are held in one array in the order of 8.4.4.2.2's search: p[-1][2N-1] .. p[-1][0], p[-1][-1], p[0][-1] .. p[2N-1][-1].
def substitute(p, avail, bd):
    """8.4.4.2.2"""
    p = np.asarray(p, np.int64)
    if not avail.any():
        return np.full(p.shape, 1 << (bd - 1), np.int64)
    idx = np.where(avail, np.arange(len(p)), -1)
    idx = np.maximum.accumulate(idx)                            # an unavailable sample takes the one before it in the search order ...
    idx[idx < 0] = int(np.argmax(avail))                        # ... p[-1][2N-1] (and what precedes the first available one) the first available
    return p[idx]


def filter_refs(p, n, mode, bd, strong_enabled, cov=None):
    """8.4.4.2.3 for luma (ChromaArrayType 1 filters no chroma reference)"""
    if mode == 1 or n == 4 or min(abs(mode - 26), abs(mode - 10)) <= HOR_VER_DIST_THRES[n]:
        return p
    c = 2 * n                                                   # index of p[-1][-1]
    if strong_enabled and n == 32:
        thr = 1 << (bd - 5)
        top_ok = abs(p[c] + p[4 * n] - 2 * p[c + n]) < thr     # Abs(p[-1][-1] + p[nTbS*2-1][-1] - 2 * p[nTbS-1][-1]) < (1 << (BitDepthY - 5))
        left_ok = abs(p[c] + p[0] - 2 * p[c - n]) < thr         # Abs(p[-1][-1] + p[-1][nTbS*2-1] - 2 * p[-1][nTbS-1]) < (1 << (BitDepthY - 5))
        if cov is not None:
            cov["smoothing", "bilinear" if top_ok and left_ok else "threshold_missed"] += 1
        if top_ok and left_ok:                                  # biIntFlag: (8-30) .. (8-34)
            q = p.copy()
            k = np.arange(63)
            q[c - 1 - k] = ((63 - k) * p[c] + (k + 1) * p[0] + 32) >> 6
            q[c + 1 + k] = ((63 - k) * p[c] + (k + 1) * p[4 * n] + 32) >> 6
            return q
    if cov is not None:
        cov["smoothing", "121"] += 1
    q = p.copy()                                                # (8-35) .. (8-39): [1 2 1], the two ends kept
    q[1:-1] = (p[:-2] + 2 * p[1:-1] + p[2:] + 2) >> 2
    return q


def predict_intra(p, n, mode, c_idx, bd):
    """8.4.4.2.4 planar, 8.4.4.2.5 DC, 8.4.4.2.6 angular over (filtered) reference samples -> n x n, [y][x]"""
    p = np.asarray(p, np.int64)
    c = 2 * n
    left = p[c - 1::-1]                                         # left[y] = p[-1][y], y = 0 .. 2N-1
    top = p[c + 1:]                                             # top[x] = p[x][-1]
    corner = p[c]
    log2 = n.bit_length() - 1
    maxv = (1 << bd) - 1
    x = np.arange(n)[None, :]
    y = np.arange(n)[:, None]
    if mode == 0:
        return ((n - 1 - x) * left[y] + (x + 1) * top[n] + (n - 1 - y) * top[x] + (y + 1) * left[n] + n) >> (log2 + 1)
    if mode == 1:
        dc = (int(top[:n].sum()) + int(left[:n].sum()) + n) >> (log2 + 1)
        out = np.full((n, n), dc, np.int64)
        if c_idx == 0 and n < 32:
            out[0, 0] = (left[0] + 2 * dc + top[0] + 2) >> 2
            out[0, 1:] = (top[1:n] + 3 * dc + 2) >> 2
            out[1:, 0] = (left[1:n] + 3 * dc + 2) >> 2
        return out
    angle = INTRA_ANGLE[mode]
    main, side = (top, left) if mode >= 18 else (left, top)
    o = 2 * n
    ref = np.zeros(4 * n + 1, np.int64)                         # ref[k] is held at ref[k + 2N], k = -2N .. 2N
    ref[o] = corner
    ref[o + 1:o + n + 1] = main[:n]
    if angle < 0:
        last = (n * angle) >> 5
        if last < -1:
            k = np.arange(last, 0)
            j = -1 + ((k * INV_ANGLE[mode] + 128) >> 8)         # position along the other side; -1 is p[-1][-1]
            ref[o + k] = np.where(j < 0, corner, side[np.maximum(j, 0)])
    else:
        ref[o + n + 1:o + 2 * n + 1] = main[n:2 * n]
    i = np.arange(n)[:, None]                                   # y for the vertical modes, x for the horizontal ones
    j = np.arange(n)[None, :]
    idx = ((i + 1) * angle) >> 5
    fact = ((i + 1) * angle) & 31
    a = ref[o + j + idx + 1]
    b = ref[np.minimum(o + j + idx + 2, 4 * n)]                 # (its weight is 0 where the index would pass the end)
    out = ((32 - fact) * a + fact * b + 16) >> 5
    if mode < 18:
        out = out.T
    if c_idx == 0 and n < 32:
        if mode == 26:
            out[:, 0] = np.clip(top[0] + ((left[:n] - corner) >> 1), 0, maxv)
        elif mode == 10:
            out[0, :] = np.clip(left[0] + ((top[:n] - corner) >> 1), 0, maxv)
    return out


# ================================================================ 8.5.3.3 inter sample prediction
def mc_luma(ref, x0, y0, n, mv, bd, cov=None):
    """8.5.3.3.3.1 for an n x n block at (x0, y0), mv in quarter samples -> predSamplesLX (14-bit intermediate); reference sample positions are
    clamped to the coded picture: xInt = Clip3(0, pic_width_in_luma_samples - 1, ...)"""
    h, w = ref.shape
    xi, yi, fx, fy = x0 + (mv[0] >> 2), y0 + (mv[1] >> 2), mv[0] & 3, mv[1] & 3
    if cov is not None:
        cov["luma_frac", fx, fy] += 1
        if xi < 0 or yi < 0 or xi + n > w or yi + n > h:
            cov["mc", "outside"] += 1
    rows = np.clip(yi - 3 + np.arange(n + 7), 0, h - 1)
    cols = np.clip(xi - 3 + np.arange(n + 7), 0, w - 1)
    blk = ref[rows[:, None], cols[None, :]].astype(np.int64)
    shift1, shift3 = min(4, bd - 8), 14 - bd
    if fx == 0 and fy == 0:
        return blk[3:3 + n, 3:3 + n] << shift3
    if fy == 0:
        return sum(FL[fx][k] * blk[3:3 + n, k:k + n] for k in range(8)) >> shift1
    if fx == 0:
        return sum(FL[fy][k] * blk[k:k + n, 3:3 + n] for k in range(8)) >> shift1
    tmp = sum(FL[fx][k] * blk[:, k:k + n] for k in range(8)) >> shift1
    return sum(FL[fy][k] * tmp[k:k + n] for k in range(8)) >> 6


def mc_chroma(ref, xc0, yc0, n, mv, bd):
    """8.5.3.3.3.2 (4:2:0: the luma vector in eighth chroma samples)"""
    h, w = ref.shape
    xi, yi, fx, fy = xc0 + (mv[0] >> 3), yc0 + (mv[1] >> 3), mv[0] & 7, mv[1] & 7
    rows = np.clip(yi - 1 + np.arange(n + 3), 0, h - 1)
    cols = np.clip(xi - 1 + np.arange(n + 3), 0, w - 1)
    blk = ref[rows[:, None], cols[None, :]].astype(np.int64)
    shift1, shift3 = min(4, bd - 8), 14 - bd
    if fx == 0 and fy == 0:
        return blk[1:1 + n, 1:1 + n] << shift3
    if fy == 0:
        return sum(FC[fx][k] * blk[1:1 + n, k:k + n] for k in range(4)) >> shift1
    if fx == 0:
        return sum(FC[fy][k] * blk[k:k + n, 1:1 + n] for k in range(4)) >> shift1
    tmp = sum(FC[fx][k] * blk[:, k:k + n] for k in range(4)) >> shift1
    return sum(FC[fy][k] * tmp[k:k + n] for k in range(4)) >> 6


def weighted_default(preds, bd):
    """8.5.3.3.4.2: one list, shift1 = 14 - bitDepth; both lists, shift2 = 15 - bitDepth, each with its rounding offset"""
    maxv = (1 << bd) - 1
    if len(preds) == 1:
        s = 14 - bd
        return np.clip((preds[0] + (1 << (s - 1))) >> s, 0, maxv)
    s = 15 - bd
    return np.clip((preds[0] + preds[1] + (1 << (s - 1))) >> s, 0, maxv)


# ================================================================ 8.7.2 deblocking
def luma_filter(P, beta, tc, bd, cov=None):
    """8.7.2.5.3 decisions and 8.7.2.5.7 filtering of edge segments: P (nseg, 4 lines, 8) = p3 p2 p1 p0 q0 q1 q2 q3; beta, tc (nseg,)"""
    maxv = (1 << bd) - 1
    p3, p2, p1, p0, q0, q1, q2, q3 = (P[:, :, k] for k in range(8))
    dp = np.abs(p2 - 2 * p1 + p0)
    dq = np.abs(q2 - 2 * q1 + q0)
    dpq0, dpq3 = dp[:, 0] + dq[:, 0], dp[:, 3] + dq[:, 3]
    on = dpq0 + dpq3 < beta

    def dsam(k, dpq):                                           # 8.7.2.5.6 with dpq = 2 * dpqK
        return ((2 * dpq < (beta >> 2)) & (np.abs(p3[:, k] - p0[:, k]) + np.abs(q0[:, k] - q3[:, k]) < (beta >> 3)) &
                (np.abs(p0[:, k] - q0[:, k]) < ((5 * tc + 1) >> 1)))
    strong = on & dsam(0, dpq0) & dsam(3, dpq3)
    normal = on & ~strong
    dep = (dp[:, 0] + dp[:, 3]) < ((beta + (beta >> 1)) >> 3)
    deq = (dq[:, 0] + dq[:, 3]) < ((beta + (beta >> 1)) >> 3)
    if cov is not None:
        cov["deblock", "strong"] += int(strong.sum())
        cov["deblock", "normal"] += int(normal.sum())
    out = P.copy()
    t = tc[:, None]
    t2, st = 2 * t, strong[:, None]
    for k, v, orig in ((3, (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3, p0), (2, (p2 + p1 + p0 + q0 + 2) >> 2, p1),
                       (1, (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3, p2), (4, (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3, q0),
                       (5, (p0 + q0 + q1 + q2 + 2) >> 2, q1), (6, (p0 + q0 + q1 + 3 * q2 + 2 * q3 + 4) >> 3, q2)):
        out[:, :, k] = np.where(st, np.clip(v, orig - t2, orig + t2), out[:, :, k])
    delta = (9 * (q0 - p0) - 3 * (q1 - p1) + 8) >> 4
    act = normal[:, None] & (np.abs(delta) < t * 10)
    delta = np.clip(delta, -t, t)
    out[:, :, 3] = np.where(act, np.clip(p0 + delta, 0, maxv), out[:, :, 3])
    out[:, :, 4] = np.where(act, np.clip(q0 - delta, 0, maxv), out[:, :, 4])
    th = t >> 1
    dpv = np.clip((((p2 + p0 + 1) >> 1) - p1 + delta) >> 1, -th, th)
    dqv = np.clip((((q2 + q0 + 1) >> 1) - q1 - delta) >> 1, -th, th)
    out[:, :, 2] = np.where(act & dep[:, None], np.clip(p1 + dpv, 0, maxv), out[:, :, 2])
    out[:, :, 5] = np.where(act & deq[:, None], np.clip(q1 + dqv, 0, maxv), out[:, :, 5])
    return out


def chroma_filter(P, tc, bd):
    """8.7.2.5.8: P (nseg, 2 lines, 4) = p1 p0 q0 q1"""
    maxv = (1 << bd) - 1
    p1, p0, q0, q1 = (P[:, :, k] for k in range(4))
    t = tc[:, None]
    delta = np.clip((((q0 - p0) << 2) + p1 - q1 + 4) >> 3, -t, t)
    out = P.copy()
    out[:, :, 1] = np.clip(p0 + delta, 0, maxv)
    out[:, :, 2] = np.clip(q0 - delta, 0, maxv)
    return out


class Grid:
    """per 4x4 luma block: what the deblocking filter asks about the two sides of an edge.  slice: SliceAddrRs; the per-slice arrays are indexed
    by it (across: slice_loop_filter_across_slices_enabled_flag, off: slice_deblocking_filter_disabled_flag, beta / tc: the offsets div2)"""

    def __init__(self, h4, w4, nslices=1):
        z = lambda v=0: np.full((h4, w4), v, np.int64)          # noqa: E731
        self.intra, self.cuid, self.nz, self.qp, self.slice, self.tile = z(), z(-1), z(), z(), z(), z()
        self.pf, self.poc, self.mvx, self.mvy = [z(), z()], [z(-1), z(-1)], [z(), z()], [z(), z()]
        self.across, self.off, self.beta, self.tc = (np.zeros(nslices, np.int64) for _ in range(4))
        self.across_tiles, self.cb_qp_offset, self.cr_qp_offset = 1, 0, 0

    def transposed(self):
        g = Grid.__new__(Grid)
        for k, v in self.__dict__.items():
            g.__dict__[k] = [a.T for a in v] if isinstance(v, list) else v.T if isinstance(v, np.ndarray) and v.ndim == 2 else v
        return g


def motion_bs(g, a, b):
    """8.7.2.4: 1 where the predictions of the two sides use different pictures, a different number of vectors, or vectors of one picture that
    differ by 4 quarter samples or more in a component (the pictures compared by identity, not by list)"""
    n_a = g.pf[0][a] + g.pf[1][a]
    n_b = g.pf[0][b] + g.pf[1][b]

    def far(la, lb):
        return (np.abs(g.mvx[la][a] - g.mvx[lb][b]) >= 4) | (np.abs(g.mvy[la][a] - g.mvy[lb][b]) >= 4)
    pa = [np.where(g.pf[k][a] == 1, g.poc[k][a], -1) for k in range(2)]
    pb = [np.where(g.pf[k][b] == 1, g.poc[k][b], -1) for k in range(2)]
    la, lb = np.where(g.pf[0][a] == 1, 0, 1), np.where(g.pf[0][b] == 1, 0, 1)         # one vector each: the list in use
    sel = lambda arr, l, s: np.where(l == 0, arr[0][s], arr[1][s])                     # noqa: E731
    one = ((np.where(la == 0, pa[0], pa[1]) != np.where(lb == 0, pb[0], pb[1])) | (np.abs(sel(g.mvx, la, a) - sel(g.mvx, lb, b)) >= 4) |
           (np.abs(sel(g.mvy, la, a) - sel(g.mvy, lb, b)) >= 4))
    same_set = ((pa[0] == pb[0]) & (pa[1] == pb[1])) | ((pa[0] == pb[1]) & (pa[1] == pb[0]))
    straight, crossed = far(0, 0) | far(1, 1), far(0, 1) | far(1, 0)
    two = ~same_set | np.where(pa[0] != pa[1], np.where(pa[0] == pb[0], straight, crossed), straight & crossed)
    return np.where(n_a != n_b, 1, np.where(n_a == 1, one, two)).astype(np.int64)


def deblock_edges(planes, g, bd, cov=None):
    """8.7.2.3-8.7.2.5 for every vertical edge of the picture on the 8x8 grid (the horizontal edges: the same on transposed arrays)"""
    y, u, v = planes
    h4, w4 = g.cuid.shape
    q = (slice(None), slice(2, w4, 2))
    p = (slice(None), slice(1, w4 - 1, 2))
    edge = g.cuid[q] != g.cuid[p]                               # coding block edges: the transform and prediction block edges of the subset
    qs = g.slice[q]
    cross_slice = qs != g.slice[p]
    filt = edge & (g.off[qs] == 0) & ~(cross_slice & (g.across[qs] == 0))      # filterEdgeFlag, and the slice of q0 must not disable the filter
    if not g.across_tiles:
        filt &= g.tile[q] == g.tile[p]
    bs = np.where((g.intra[q] == 1) | (g.intra[p] == 1), 2, np.where((g.nz[q] == 1) | (g.nz[p] == 1), 1, motion_bs(g, q, p)))
    bs = np.where(filt, bs, 0)
    if cov is not None:
        cov["deblock", "slice_edge_unfiltered"] += int((edge & cross_slice & (g.across[qs] == 0)).sum())
        cov["deblock", "bs1"] += int((bs == 1).sum())
        cov["deblock", "bs2"] += int((bs == 2).sum())
    ii, jj = np.nonzero(bs)
    if len(ii) == 0:
        return
    jq = 2 + 2 * jj                                             # 4x4 column of q0
    bsv = bs[ii, jj]
    sq = g.slice[ii, jq]
    qpl = (g.qp[ii, jq] + g.qp[ii, jq - 1] + 1) >> 1
    beta = BETA_TABLE[np.clip(qpl + 2 * g.beta[sq], 0, 51)] * (1 << (bd - 8))
    tc = TC_TABLE[np.clip(qpl + 2 * (bsv - 1) + 2 * g.tc[sq], 0, 53)] * (1 << (bd - 8))
    rows = (4 * ii[:, None] + np.arange(4))[:, :, None]
    cols = (4 * jq[:, None] + np.arange(-4, 4))[:, None, :]
    y[rows, cols] = luma_filter(y[rows, cols].astype(np.int64), beta, tc, bd, cov)
    ch = (bsv == 2) & ((4 * jq) % 16 == 0)                      # chroma: bS 2 on the 8-sample chroma grid
    if not ch.any():
        return
    if cov is not None:
        cov["deblock", "chroma"] += int(ch.sum())
    ii, jq, qpl, sq = ii[ch], jq[ch], qpl[ch], sq[ch]
    rows = (2 * ii[:, None] + np.arange(2))[:, :, None]
    cols = (2 * jq[:, None] + np.arange(-2, 2))[:, None, :]
    for plane, off in ((u, g.cb_qp_offset), (v, g.cr_qp_offset)):
        qpc = np.array([qpc_from_qpi(int(k) + off) for k in qpl], np.int64)        # QpC from ((QpQ + QpP + 1) >> 1) + cQpPicOffset
        tc = TC_TABLE[np.clip(qpc + 2 + 2 * g.tc[sq], 0, 53)] * (1 << (bd - 8))
        plane[rows, cols] = chroma_filter(plane[rows, cols].astype(np.int64), tc, bd)


def deblock(planes, g, bd, cov=None):
    """8.7.2: all vertical edges of the picture, then all horizontal edges on the result (planes are changed in place)"""
    deblock_edges(planes, g, bd, cov)
    deblock_edges([p.T for p in planes], g.transposed(), bd, cov)


# ================================================================ 8.7.3 SAO
EO_DIRS = {0: ((0, -1), (0, 1)), 1: ((-1, 0), (1, 0)), 2: ((-1, -1), (1, 1)), 3: ((-1, 1), (1, -1))}    # (dy, dx) of the two neighbours


def sao_plane(dbk, c, bd, ctb_log2, prm, region=None, cov=None):
    """8.7.3.2 for one colour component: dbk the deblocked plane (the neighbours are read from it); ctb_log2 the CTB size in this component's
    samples; prm per CTB in raster order: None or {"type", "eo_class", "band_pos", "offset"} as the syntax reader holds them (SaoTypeIdx and
    the class shared by Cb and Cr).  region, when given, is (slice per CTB, decoding order of each slice's first CTB, the across-slices flag
    per slice, tile per CTB, loop_filter_across_tiles_enabled_flag)."""
    h, w = dbk.shape
    cs = 1 << ctb_log2
    wc = (w + cs - 1) >> ctb_log2
    yy, xx = np.mgrid[0:h, 0:w]
    ctb = (yy >> ctb_log2) * wc + (xx >> ctb_log2)
    n = len(prm)
    typ, cls, band = (np.zeros(n, np.int64) for _ in range(3))
    off = np.zeros((n, 5), np.int64)                            # SaoOffsetVal[0..4] (<< (bitDepth - Min(bitDepth, 10)) = << 0 at 8 and 10 bit)
    for rs, pr in enumerate(prm):
        if pr is not None:
            typ[rs], cls[rs], band[rs] = pr["type"][min(c, 1)], pr["eo_class"][min(c, 1)], pr["band_pos"][c]
            off[rs, 1:] = pr["offset"][c]
    t = typ[ctb]
    rec = dbk.astype(np.int64)
    out = rec.copy()
    maxv = (1 << bd) - 1
    m = t == 1                                                  # band offset: bandTable[(k + sao_band_position) & 31] = k + 1, bandShift = bitDepth - 5
    if m.any():
        k = ((rec >> (bd - 5)) - band[ctb]) & 31
        bidx = np.where(k < 4, k + 1, 0)
        out[m] = np.clip(rec + off[ctb, bidx], 0, maxv)[m]
        if cov is not None:
            cov["sao_band", c] += 1
            if (band[np.unique(ctb[m])] > 28).any():
                cov["sao_band_wrap", c] += 1
    for e in range(4):
        sel = (t == 2) & (cls[ctb] == e)
        if not sel.any():
            continue
        if cov is not None:
            cov["sao_edge", c, e] += 1
        val = np.zeros((h, w), np.int64)
        ok = np.ones((h, w), bool)
        for dy, dx in EO_DIRS[e]:
            ny, nx = yy + dy, xx + dx
            ok &= (ny >= 0) & (ny < h) & (nx >= 0) & (nx < w)   # no neighbour outside the picture: SaoOffsetVal 0
            ny, nx = np.clip(ny, 0, h - 1), np.clip(nx, 0, w - 1)
            if region is not None:
                sl_ctb, order, across, tile_ctb, across_tiles = region
                s0, s1 = sl_ctb[ctb], sl_ctb[ctb[ny, nx]]
                later = np.where(order[s1] > order[s0], s1, s0)             # the slice of whichever sample comes later in decoding order
                ok &= ~((s0 != s1) & (across[later] == 0))
                if not across_tiles:
                    ok &= tile_ctb[ctb] == tile_ctb[ctb[ny, nx]]
            val += np.sign(rec - rec[ny, nx])
        idx = val + 2
        idx = np.where(idx == 2, 0, np.where(idx < 2, idx + 1, idx))          # edgeIdx 0, 1, 2 -> 1, 2, 0
        idx = np.where(ok, idx, 0)
        if cov is not None:
            cov["sao_edge_kept", c] += int((sel & ~ok).sum())
        out[sel] = np.clip(rec + off[ctb, idx], 0, maxv)[sel]
    return out


# ================================================================ pictures
def decode_order(pic, lay):
    """the CUs of a picture in decoding order, CTBs in tile scan and z-order inside: [(x0, y0, log2)]"""
    out = []
    log2g = pic.cu["log2"]

    def quad(x, y, log2):
        if x >= pic.w or y >= pic.h:
            return
        if log2 > int(log2g[y >> 3, x >> 3]):
            hh = 1 << (log2 - 1)
            for k in range(4):
                quad(x + (k & 1) * hh, y + (k >> 1) * hh, log2 - 1)
        else:
            out.append((x, y, log2))
    for ts in range(lay.wc * lay.hc):
        rs = lay.ts2rs[ts]
        quad((rs % lay.wc) << 5, (rs // lay.wc) << 5, 5)
    return out


def reconstruct_picture(st, pic, dpb, cov):
    """8.4, 8.5, 8.6 per CU in decoding order, then 8.7.2 and 8.7.3 -> (final, before deblocking, after deblocking), planes as uint16"""
    sl = {s["address"]: s["header"] for s in pic.slices}
    pps = st.pps[pic.slices[0]["pps_id"]]
    sps = st.sps[pps["sps_id"]]
    bd, lay = sps["bit_depth_luma"], pic.layout
    h, w = pic.h, pic.w
    nctb = lay.wc * lay.hc
    planes = [np.zeros((h, w), np.int64), np.zeros((h // 2, w // 2), np.int64), np.zeros((h // 2, w // 2), np.int64)]
    h4, w4 = h >> 2, w >> 2
    g = Grid(h4, w4, nctb)
    for a, hdr in sl.items():
        g.across[a] = hdr["slice_loop_filter_across_slices_enabled_flag"]
        g.off[a] = hdr["slice_deblocking_filter_disabled_flag"]
        if "beta_offset_div2" in hdr:                           # slice_beta_offset_div2 / slice_tc_offset_div2, else the PPS's
            g.beta[a], g.tc[a] = hdr["beta_offset_div2"], hdr["tc_offset_div2"]
        else:
            g.beta[a], g.tc[a] = pps.get("beta_offset_div2", 0), pps.get("tc_offset_div2", 0)
    g.across_tiles = pps.get("loop_filter_across_tiles_enabled_flag", 1)
    g.cb_qp_offset, g.cr_qp_offset = pps["cb_qp_offset"], pps["cr_qp_offset"]
    tile_ctb = np.array([lay.tile_of_rs(rs) for rs in range(nctb)], np.int64)
    sl_ctb = np.array(pic.ctb_slice, np.int64)
    ctb4 = (np.arange(h4)[:, None] >> 3) * lay.wc + (np.arange(w4)[None, :] >> 3)
    g.slice, g.tile = sl_ctb[ctb4], tile_ctb[ctb4]
    done = np.zeros((h4, w4), bool)
    qps = {}
    for a, hdr in sl.items():                                   # 8.6.1 without cu_qp_delta: QpY = SliceQpY
        qpy, off = hdr["slice_qp"], 6 * (bd - 8)
        qc = [qpc_from_qpi(min(max(-off, qpy + po + so), 57)) + off
              for po, so in ((pps["cb_qp_offset"], hdr["slice_cb_qp_offset"]), (pps["cr_qp_offset"], hdr["slice_cr_qp_offset"]))]
        qps[a] = (qpy, qpy + off, qc[0], qc[1])
    maxv = (1 << bd) - 1
    strong = sps["strong_intra_smoothing_enabled_flag"]
    cu = pic.cu

    def intra_tb(c, x0, y0, n, mode):
        s = 2 if c else 1
        plane = planes[c]
        ph, pw = plane.shape
        k = np.arange(4 * n + 1)
        xs = np.where(k < 2 * n, -1, k - 2 * n - 1) + x0
        ys = np.where(k < 2 * n, 2 * n - 1 - k, -1) + y0
        inside = (xs >= 0) & (ys >= 0) & (xs < pw) & (ys < ph)
        cy, cx = np.clip(ys, 0, ph - 1), np.clip(xs, 0, pw - 1)
        i4, j4 = (cy * s) >> 2, (cx * s) >> 2
        b4 = ((y0 * s) >> 2, (x0 * s) >> 2)
        # 6.4.1: decoded already (z-scan order), in the same slice and the same tile
        avail = inside & done[i4, j4] & (g.slice[i4, j4] == g.slice[b4]) & (g.tile[i4, j4] == g.tile[b4])
        p = substitute(plane[cy, cx], avail, bd)
        if c == 0:
            p = filter_refs(p, n, mode, bd, strong, cov)
        cov["intra", c, n, mode] += 1
        return predict_intra(p, n, mode, c, bd)

    for x0, y0, log2 in decode_order(pic, lay):
        n = 1 << log2
        by, bx = y0 >> 3, x0 >> 3
        addr = int(cu["slice"][by, bx])
        qpy, qy, qcb, qcr = qps[addr]
        intra = not cu["inter"][by, bx]
        b4 = (slice(y0 >> 2, (y0 + n) >> 2), slice(x0 >> 2, (x0 + n) >> 2))
        g.cuid[b4], g.qp[b4], g.intra[b4] = y0 * w + x0, qpy, int(intra)
        xc, yc, nc = x0 >> 1, y0 >> 1, n >> 1
        if intra:
            imodes = [int(m) for m in cu["imode"][by, bx]]
            cmode = int(cu["cmode"][by, bx])
            if cu["nxn"][by, bx]:
                for k in range(4):
                    xb, yb = x0 + 4 * (k & 1), y0 + 4 * (k >> 1)
                    pred = intra_tb(0, xb, yb, 4, imodes[k])
                    lv = pic.coef[0][yb:yb + 4, xb:xb + 4]
                    cov["dst"] += 1                             # DST-VII: intra luma 4x4 only
                    planes[0][yb:yb + 4, xb:xb + 4] = np.clip(pred + residual(lv, qy, bd, dst=True), 0, maxv)
                    done[yb >> 2, xb >> 2] = True
                    g.nz[yb >> 2, xb >> 2] = int(lv.any())
                nc = 4
            else:
                pred = intra_tb(0, x0, y0, n, imodes[0])
                lv = pic.coef[0][y0:y0 + n, x0:x0 + n]
                planes[0][y0:y0 + n, x0:x0 + n] = np.clip(pred + residual(lv, qy, bd), 0, maxv)
                g.nz[b4] = int(lv.any())
            for c, q in ((1, qcb), (2, qcr)):
                pred = intra_tb(c, xc, yc, nc, cmode)
                lv = pic.coef[c][yc:yc + nc, xc:xc + nc]
                planes[c][yc:yc + nc, xc:xc + nc] = np.clip(pred + residual(lv, q, bd), 0, maxv)
        else:
            hdr = sl[addr]
            pf = (int(cu["pf0"][by, bx]), int(cu["pf1"][by, bx]))
            mvs = ((int(cu["mv0x"][by, bx]), int(cu["mv0y"][by, bx])), (int(cu["mv1x"][by, bx]), int(cu["mv1y"][by, bx])))
            preds = [[], [], []]
            for lx in range(2):
                if not pf[lx]:
                    continue
                poc = hdr["ref_pocs"][lx]                       # RefPicListX[0] (8.3.4), one picture per list
                ref = dpb[poc]
                g.pf[lx][b4], g.poc[lx][b4], g.mvx[lx][b4], g.mvy[lx][b4] = 1, poc, mvs[lx][0], mvs[lx][1]
                preds[0].append(mc_luma(ref[0], x0, y0, n, mvs[lx], bd, cov))
                for c in (1, 2):
                    preds[c].append(mc_chroma(ref[c], xc, yc, nc, mvs[lx], bd))
            cov["inter", "bi" if len(preds[0]) == 2 else "uni"] += 1
            lv = pic.coef[0][y0:y0 + n, x0:x0 + n]
            planes[0][y0:y0 + n, x0:x0 + n] = np.clip(weighted_default(preds[0], bd) + residual(lv, qy, bd), 0, maxv)
            g.nz[b4] = int(lv.any())
            for c, q in ((1, qcb), (2, qcr)):
                lvc = pic.coef[c][yc:yc + nc, xc:xc + nc]
                planes[c][yc:yc + nc, xc:xc + nc] = np.clip(weighted_default(preds[c], bd) + residual(lvc, q, bd), 0, maxv)
        done[b4] = True
    pre = [p.astype(np.uint16) for p in planes]
    deblock(planes, g, bd, cov)
    dbk = [p.astype(np.uint16) for p in planes]
    if sps["sao_enabled_flag"]:
        order = np.zeros(nctb, np.int64)
        for a in sl:
            order[a] = lay.rs2ts[a]
        region = (sl_ctb, order, g.across, tile_ctb, g.across_tiles)
        for c in range(3):
            prm = [pr if pr is not None and sl[pic.ctb_slice[rs]]["slice_sao_chroma_flag" if c else "slice_sao_luma_flag"] else None
                   for rs, pr in enumerate(pic.sao)]
            planes[c] = sao_plane(planes[c], c, bd, 5 - (c > 0), prm, region, cov)
    return [p.astype(np.uint16) for p in planes], pre, dbk


def reconstruct(stream, stats=None):
    """stream: bytes or a tests.hevc_syntax.Stream -> [(poc, y, u, v)] in decoding order"""
    st = S.parse_stream(stream) if isinstance(stream, (bytes, bytearray)) else stream
    cov = collections.Counter()
    out, pres, dbks, hashes = [], [], [], []
    dpb = {}
    for pic in st.pictures:
        dpb = {poc: v for poc, v in dpb.items() if poc in pic.rps_all}      # 8.3.2: what the RPS does not name is no longer referenced
        final, pre, dbk = reconstruct_picture(st, pic, dpb, cov)
        if pic.nal_type != 0:                                   # TRAIL_N: a sub-layer non-reference picture is never referenced
            dpb[pic.poc] = final
        out.append((pic.poc, *final))
        pres.append(pre)
        dbks.append(dbk)
        if pic.hash is None:
            hashes.append(None)
        else:
            kind, vals = pic.hash
            bd = st.sps[st.pps[pic.slices[0]["pps_id"]]["sps_id"]]["bit_depth_luma"]
            hashes.append((kind, vals, H.picture_hash(final, bd, kind)))
    if stats is not None:
        stats.update(pre=pres, dbk=dbks, hash=hashes, cov=cov)
    return out
