"""A third statement of the intra PLAN: the luma and chroma intra prediction modes of all 21 quadtree nodes of every CTU and the quadtree itself, as
`mihevc_k_intra_plan` returns them (include/mihevc.h, `mihevc_intra_plan`).

Written from the documents alone: DESIGN.md §6 ("Decision rules, in words", the intra plan items), the comments of include/mihevc.h and H.265 6.4.1 / 6.5.1
(availability, tile boundaries), 8.4.2 (candModeList) and 8.4.4.2 (reference samples and prediction; the latter through tests/hevc_recon.py, which is
written from the same clauses).  Not from hevc_amd/csrc/kernels/intra.h and not from oracle/hevc_oracle.c, which are one author's two statements of the
same rules and share their structure (a packed (cost << 6 | mode) key, per-tile SATD accumulation, one RD pass per level).  Everything here is brute
force instead: every node is predicted in every mode as a whole block, the SATD is taken of the whole difference, every candidate is priced into an
explicitly ordered array and `argmin` takes the first minimum.

What does not depend on the cost parameters (reference samples, the SATD of every node in every mode) is kept per picture, so one picture can be planned
at several QPs for the price of one.

Imports: numpy, the standard library, tests/hevc_recon.py (8.4.4.2), tests/hevc_analysis.py (node geometry) and tests/transform_ref.py (K3)
(tests/test_syntax_independent.py checks it)."""
import collections

import numpy as np

from tests import hevc_analysis as A
from tests import hevc_recon as R
from tests import transform_ref as K3

CTU = 32
NODES = A.NODES                                  # (x, y, size) of node 0..20 inside the CTU
NODE_AT = {g: i for i, g in enumerate(NODES)}
PLAN_DTYPE = np.dtype([("chosen", "u1", (21,)), ("mode", "u1", (21,)), ("cmode", "u1", (21,)), ("pad", "u1")])      # include/mihevc.h, mihevc_intra_plan
PLANAR, DC, HOR, VER = 0, 1, 10, 26
CHROMA_BASES = (PLANAR, VER, HOR, DC)            # the four explicit candidates behind DM, in the order of the rule
R_SB, R_TU = 143, 30                             # 1/16 bit: a 4x4 sub-block with a level; a transform unit with a level


def hadamard(n):
    h = np.ones((1, 1), np.int64)
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


def satd(diff, tile):
    """diff: (..., n, n).  The block is cut into tile x tile pieces; each piece costs sum |H d H^T| normalised on its own — (s + 2) >> 2 for 8x8 pieces,
    (s + 1) >> 1 for 4x4 — and the pieces are added."""
    d = np.asarray(diff, np.int64)
    n = d.shape[-1]
    k = n // tile
    d = d.reshape(d.shape[:-2] + (k, tile, k, tile)).swapaxes(-3, -2)          # (..., piece row, piece column, tile, tile)
    h = hadamard(tile)
    raw = np.abs(h @ d @ h.T).sum(axis=(-1, -2))
    per = (raw + 2) >> 2 if tile == 8 else (raw + 1) >> 1
    return per.sum(axis=(-1, -2))


def z_index(x, y):
    """z-scan position of the 4x4 unit that holds sample (x, y) of a CTU (6.5.2): the bits of its column and row interleaved, column lowest"""
    ux, uy = np.asarray(x) >> 2, np.asarray(y) >> 2
    z = np.zeros_like(ux)
    for b in range(3):
        z = z + (((ux >> b) & 1) << (2 * b)) + (((uy >> b) & 1) << (2 * b + 1))
    return z


def tile_bounds(n_ctb, n_tiles):
    """6.5.1, uniform spacing: first CTB of tile i = (i * n_ctb) / n_tiles, i = 0 .. n_tiles"""
    return [i * n_ctb // n_tiles for i in range(n_tiles + 1)]


def cand_mode_list(a, b, cov=None):
    """8.4.2 (8-21 .. 8-27) from candIntraPredModeA (left) and B (above)"""
    if a == b:
        if a < 2:
            kind, out = "equal, non-angular", [PLANAR, DC, VER]
        else:
            kind, out = "equal, angular", [a, 2 + ((a + 29) % 32), 2 + ((a - 2 + 1) % 32)]
    else:
        c = PLANAR if PLANAR not in (a, b) else DC if DC not in (a, b) else VER
        kind, out = "different", [a, b, c]
    if cov is not None:
        cov["cand_from", kind] += 1
    return out


def mode_bits(cand, mode):
    return 2 if mode == cand[0] else 3 if mode in cand[1:] else 6


def level_rate(a):
    """1/16 bit of one non-zero level of magnitude a"""
    return 33 if a == 1 else 50 if a == 2 else 53 + 27 * (int(a - 1).bit_length() - 1)


def coefficient_bits(levels):
    """1/16 bit of one transform block's levels: per 4x4 sub-block that holds a level 143 + the levels' rates; 30 more when the block holds any"""
    lv = np.abs(np.asarray(levels, np.int64))
    n = lv.shape[0]
    bits = 0
    for y in range(0, n, 4):
        for x in range(0, n, 4):
            sb = lv[y:y + 4, x:x + 4]
            if sb.any():
                bits += R_SB + sum(level_rate(a) for a in sb[sb > 0].tolist())
    return bits + R_TU if bits else 0


class IntraPlanModel:
    """One picture (Y, Cb, Cr planes of the coded size, 4:2:0) and its tile grid; plan() decides it for one set of cost parameters."""

    def __init__(self, planes, bit_depth, tile_cols=1, tile_rows=1, cov=None):
        self.p = [np.asarray(x).astype(np.int64) for x in planes]
        self.h, self.w = self.p[0].shape
        assert self.w % 8 == 0 and self.h % 8 == 0 and self.p[1].shape == (self.h // 2, self.w // 2) == self.p[2].shape
        self.bd = bit_depth
        self.wc, self.hc = (self.w + CTU - 1) // CTU, (self.h + CTU - 1) // CTU
        self.col_bd, self.row_bd = tile_bounds(self.wc, max(tile_cols, 1)), tile_bounds(self.hc, max(tile_rows, 1))
        self.cov = cov if cov is not None else collections.Counter()
        self._refs, self._luma, self._chroma = {}, {}, {}

    # ---------------------------------------------------------------- reference samples (from the SOURCE picture)
    def tile_box(self, cx, cy):
        """luma sample bounds (x_lo, x_hi, y_lo, y_hi) of the tile that holds CTU (cx, cy)"""
        i = max(k for k in range(len(self.col_bd) - 1) if self.col_bd[k] <= cx)
        j = max(k for k in range(len(self.row_bd) - 1) if self.row_bd[k] <= cy)
        return self.col_bd[i] * CTU, self.col_bd[i + 1] * CTU, self.row_bd[j] * CTU, self.row_bd[j + 1] * CTU

    def order(self, lx, ly):
        """decoding order of the 4x4 unit at luma (lx, ly) among the units of ONE tile: CTBs in raster order, z-scan inside the CTB"""
        return ((ly >> 5) * self.wc + (lx >> 5)) * 64 + z_index(lx & 31, ly & 31)

    def references(self, c, x, y, n):
        """the 4n + 1 substituted reference samples of the n x n block at (x, y) of plane c, in the order of 8.4.4.2.2's search.  A neighbouring sample
        is available when it lies in the picture, in the block's tile, and in a 4x4 unit that precedes the block's own in decoding order (6.4.1)."""
        key = (c, x, y, n)
        if key in self._refs:
            return self._refs[key]
        sh = 1 if c else 0
        k = np.arange(2 * n)
        xs = np.concatenate([np.full(2 * n, x - 1), [x - 1], x + k])
        ys = np.concatenate([y + 2 * n - 1 - k, [y - 1], np.full(2 * n, y - 1)])
        lx, ly = xs << sh, ys << sh
        bx, by = x << sh, y << sh
        x_lo, x_hi, y_lo, y_hi = self.tile_box(bx >> 5, by >> 5)
        in_pic = (lx >= 0) & (ly >= 0) & (lx < self.w) & (ly < self.h)
        in_tile = (lx >= x_lo) & (lx < x_hi) & (ly >= y_lo) & (ly < y_hi)
        earlier = self.order(np.clip(lx, 0, self.w - 1), np.clip(ly, 0, self.h - 1)) < self.order(bx, by)
        avail = in_pic & in_tile & earlier
        self.cov["unavailable", "picture"] += int((~in_pic).sum())
        self.cov["unavailable", "tile"] += int((in_pic & ~in_tile).sum())
        self.cov["unavailable", "z-order"] += int((in_pic & in_tile & ~earlier).sum())
        plane = self.p[c]
        raw = np.where(avail, plane[np.clip(ys, 0, plane.shape[0] - 1), np.clip(xs, 0, plane.shape[1] - 1)], 0)
        out = R.substitute(raw, avail, self.bd)
        self._refs[key] = out
        return out

    # ---------------------------------------------------------------- what does not depend on the cost parameters
    def luma_satd(self, gx, gy, n):
        """SATD of the n x n luma block at (gx, gy) against its prediction in each of the 35 modes"""
        key = (gx, gy, n)
        if key not in self._luma:
            p = self.references(0, gx, gy, n)
            src = self.p[0][gy:gy + n, gx:gx + n]
            pred = np.stack([R.predict_intra(R.filter_refs(p, n, m, self.bd, True, self.cov), n, m, 0, self.bd) for m in range(35)])
            self._luma[key] = satd(src - pred, 8)
        return self._luma[key]

    def chroma_satd(self, gx, gy, n, mode):
        """Cb + Cr SATD of the chroma blocks of the n x n luma block at (gx, gy) in chroma prediction mode `mode`"""
        key = (gx, gy, n, mode)
        if key not in self._chroma:
            nc, total = n // 2, 0
            for c in (1, 2):
                pred = R.predict_intra(self.references(c, gx // 2, gy // 2, nc), nc, mode, c, self.bd)
                total += int(satd(self.p[c][gy // 2:gy // 2 + nc, gx // 2:gx // 2 + nc] - pred, 8 if nc >= 8 else 4))
            self._chroma[key] = total
        return self._chroma[key]

    # ---------------------------------------------------------------- the RD cost of a node with its modes
    def node_cost(self, gx, gy, n, mode, cmode, mbits, qp, qp_c, lambda_q4):
        """(J, SSE, bits in 1/16 bit): every plane predicted from the SOURCE neighbourhood as one block, its residual through K3 as ONE transform block of
        the plane's size (DCT, intra rounding; luma at qp, chroma at qp_c), SSE of source against clip(prediction + reconstructed residual)"""
        sse, bits = 0, 16 * mbits + 16 + 24 + (32 if cmode != mode else 0)
        for c in range(3):
            x, y, m, q, k = (gx, gy, n, qp, mode) if c == 0 else (gx // 2, gy // 2, n // 2, qp_c, cmode)
            p = self.references(c, x, y, m)
            if c == 0:
                p = R.filter_refs(p, m, k, self.bd, True)
            pred = R.predict_intra(p, m, k, c, self.bd)
            src = self.p[c][y:y + m, x:x + m]
            lvl, rec = K3.reference((src - pred)[None], m.bit_length() - 1, q, self.bd, True)
            d = src - np.clip(pred + rec[0], 0, (1 << self.bd) - 1)
            sse += int((d * d).sum())
            bits += coefficient_bits(lvl[0])
        return (sse << 4) + ((lambda_q4 * bits) >> 4), sse, bits

    # ---------------------------------------------------------------- the plan
    def plan(self, qp, qp_c, lambda_sad_q4, lambda_q4, chroma_modes=1, detail=None, only=None):
        """-> one PLAN_DTYPE record per CTU in raster order.  detail: a list that receives, per CTU, a dict node -> (luma costs[35], chroma costs[5] or
        None, J, SSE, bits) of the nodes inside the picture.  only: the CTUs to plan (the plan of a CTU depends on no other CTU); the others stay zero."""
        out = np.zeros(self.wc * self.hc, PLAN_DTYPE)
        for ctu in range(self.wc * self.hc) if only is None else sorted(only):
            x0, y0 = ctu % self.wc * CTU, ctu // self.wc * CTU
            valid = [x0 + x + n <= self.w and y0 + y + n <= self.h for x, y, n in NODES]
            mode, cmode, J, info = {}, {}, {}, {}
            for nd, (x, y, n) in enumerate(NODES):       # within a level this is the z-order: left and above come first
                if not valid[nd]:
                    self.cov["invalid node"] += 1
                    continue
                left = mode[NODE_AT[(x - n, y, n)]] if x > 0 else DC
                above = mode[NODE_AT[(x, y - n, n)]] if y > 0 else DC
                cand = cand_mode_list(left, above, self.cov)
                bits = np.array([mode_bits(cand, m) for m in range(35)], np.int64)
                lcost = (self.luma_satd(x0 + x, y0 + y, n) << 4) + lambda_sad_q4 * bits
                m = int(np.argmin(lcost))                                       # modes in ascending order: the lowest of equal costs
                self.cov["luma", m] += 1
                cm, ccost = m, None
                if chroma_modes:
                    cmodes = [m] + [34 if b == m else b for b in CHROMA_BASES]   # DM, planar, 26, 10, DC; 34 where one of the four IS the luma mode
                    ccost = np.array([(self.chroma_satd(x0 + x, y0 + y, n, k) << 4) + lambda_sad_q4 * (1 if i == 0 else 3) for i, k in enumerate(cmodes)], np.int64)
                    i = int(np.argmin(ccost))                                   # DM first: it wins ties
                    cm = cmodes[i]
                    self.cov["chroma", ("DM", "planar", "vertical", "horizontal", "DC")[i]] += 1
                    if i and cm == 34:
                        self.cov["chroma", "34 for the luma mode"] += 1
                mode[nd], cmode[nd] = m, cm
                J[nd], sse, nbits = self.node_cost(x0 + x, y0 + y, n, m, cm, int(bits[m]), qp, qp_c, lambda_q4)
                info[nd] = (lcost, ccost, J[nd], sse, nbits)
            # the tree, bottom-up
            lam = lambda_q4
            use16, j16 = [False] * 4, [0] * 4
            for q in range(4):
                kids = [5 + 4 * q + k for k in range(4) if valid[5 + 4 * q + k]]
                if not kids:
                    continue                                                     # a quadrant outside the picture costs nothing
                split = lam + sum(J[k] for k in kids)
                use16[q] = valid[1 + q] and J[1 + q] + lam <= split             # the whole node wins ties
                j16[q] = J[1 + q] + lam if use16[q] else split
            use32 = valid[0] and J[0] + lam <= lam + sum(j16)
            o = out[ctu]
            for nd in range(21):
                if not valid[nd]:
                    continue                                                     # chosen, mode, cmode stay 0
                o["mode"][nd], o["cmode"][nd] = mode[nd], cmode[nd]
                leaf = use32 if nd == 0 else (not use32 and use16[nd - 1]) if nd < 5 else (not use32 and not use16[(nd - 5) >> 2])
                o["chosen"][nd] = int(leaf)
                if leaf:
                    self.cov["leaf", NODES[nd][2]] += 1
            if detail is not None:
                detail.append(info)
        return out


def plan_picture(planes, bit_depth, qp, qp_c, lambda_sad_q4, lambda_q4, tile_cols=1, tile_rows=1, chroma_modes=1, cov=None, detail=None):
    return IntraPlanModel(planes, bit_depth, tile_cols, tile_rows, cov).plan(qp, qp_c, lambda_sad_q4, lambda_q4, chroma_modes, detail)
