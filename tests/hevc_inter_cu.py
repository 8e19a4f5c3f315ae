"""A third statement of the inter CTU program: what `mihevc_k_inter_frame` / `mihevc_k_b_frame` decide AFTER the integer search — the quadtree of
every CTU, the half- and quarter-sample vector of every CU, the list-0 / list-1 / bi-prediction choice of B pictures, the RD zero-out of inter TUs,
the RD zero-out of their 4x4 coefficient groups (`rdo_cg`, DESIGN.md §6b: `group_zero_out`), sign data hiding behind it, the CU records, levels, pre-deblock reconstruction
and the picture's rate estimate.

Written from the documents alone: DESIGN.md §6 ("Decision rules of the inter CTU program, in words"), the comments of include/mihevc.h
(`mihevc_cu_rec`) and H.265 8.5.3.3.3 / 8.5.3.3.4.2 through tests/hevc_recon.py.  Not from hevc_amd/csrc/kernels/inter.h and not from
oracle/hevc_oracle.c, which are one author's two statements of the same rules and share their structure (a ring table, a packed
(cost << 4 | position) key, tile sums shared between nodes with equal vectors).  Everything here is brute force instead: every node's whole
prediction block comes from `mc_luma`, the Hadamard transform is a matrix product, every candidate is priced in a plain loop into a list and the
first minimum is taken.

Imports: numpy, the standard library, tests/hevc_analysis.py (node geometry, mvd bits, the integer search that `integer_table` starts from), tests/hevc_recon.py (8.5.3.3.3, default weighted
prediction), tests/transform_ref.py (K3) and tests/sdh_ref.py (the sign data hiding rule) (tests/test_syntax_independent.py checks it)."""
import collections

import numpy as np

from tests import hevc_analysis as A
from tests import hevc_recon as R
from tests import sdh_ref as SDH
from tests import transform_ref as K3

CTU = 32
NODES = A.NODES
# include/mihevc.h, mihevc_cu_rec
CU_DTYPE = np.dtype([("log2_size", "u1"), ("flags", "u1"), ("chroma_mode", "u1"), ("qp", "u1"), ("intra_mode", "u1", (4,)),
                     ("mvx", "<i2"), ("mvy", "<i2"), ("cbf_y4", "u1"), ("pad", "u1", (3,))])
F_INTER, F_CBF = 1, (2, 4, 8)
F_L1, F_NOL0 = 32, 64
RING = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))     # candidates 1..8; candidate 0 is the centre
R_SB, R_TU, R_CU = 143, 30, 80                                                     # 1/16 bit
L0, L1, BI = 0, 1, 2

H8 = np.array([[-1 if bin(i & j).count("1") & 1 else 1 for j in range(8)] for i in range(8)], np.int64)


def satd(diff):
    """diff: n x n, n a multiple of 8.  Cut into 8x8 tiles; each tile costs sum |H d H^T| normalised on its own, (s + 2) >> 2; the tiles are added."""
    d = np.asarray(diff, np.int64)
    total = 0
    for y in range(0, d.shape[0], 8):
        for x in range(0, d.shape[1], 8):
            total += (int(np.abs(H8 @ d[y:y + 8, x:x + 8] @ H8.T).sum()) + 2) >> 2
    return total


def mv_bits(mv, centre):
    return A.mvd_bits(mv[0] - 4 * centre[0]) + A.mvd_bits(mv[1] - 4 * centre[1])


def rows_inside(y, n, my, h, top, bottom):
    """may a block of n luma rows at picture row y use the vertical vector my (quarter samples) when the picture's first row (top) / last row
    (bottom) is a slice edge?  With a vertical fraction the 8-tap luma filter reads 3 rows above and 4 below the block's displaced rows; the chroma
    block (n / 2 rows at y / 2, vector in eighth samples) reads 1 above and 2 below when ITS fraction is not zero."""
    l0, l1 = y + (my >> 2), y + (my >> 2) + n - 1
    if my & 3:
        l0, l1 = l0 - 3, l1 + 4
    c0, c1 = (y >> 1) + (my >> 3), (y >> 1) + (my >> 3) + (n >> 1) - 1
    if my & 7:
        c0, c1 = c0 - 1, c1 + 2
    if top and (l0 < 0 or c0 < 0):
        return False
    if bottom and (l1 > h - 1 or c1 > (h >> 1) - 1):
        return False
    return True


def clamp_centre_y(sy, y0, me_range, h, top, bottom):
    """the centre of a CTU is pulled back so that the whole +-me_range window keeps the CTU's rows (those inside the picture) inside the slice"""
    rows = min(CTU, h - y0)
    if bottom:
        sy = min(sy, h - (y0 + rows) - me_range)
    if top:
        sy = max(sy, me_range - y0)
    return sy


def level_rate(a):
    return 33 if a == 1 else 50 if a == 2 else 53 + 27 * (int(a - 1).bit_length() - 1)


def sub_block_bits(levels):
    """1/16 bit of one transform block's levels: per 4x4 sub-block that holds a level, 143 + the rates of its levels"""
    lv = np.abs(np.asarray(levels, np.int64))
    bits = 0
    for y in range(0, lv.shape[0], 4):
        for x in range(0, lv.shape[1], 4):
            sb = lv[y:y + 4, x:x + 4]
            if sb.any():
                bits += R_SB + sum(level_rate(a) for a in sb[sb > 0].tolist())
    return bits


def group_zero_out(coef, lvl, deq, log2n, bit_depth, lambda_q4, k):
    """DESIGN.md §6b (`rdo_cg`), include/mihevc.h: the RD zero-out of the 4x4 coefficient groups of one inter TU.  coef: its forward coefficients,
    lvl: its levels, deq: its scaled levels (clipped to 16 bit), all n x n.  Dropping a group adds D = sum r (2 c - r) of squared coefficient error over
    its non-zero levels and saves its levels' bits + one sub-block of the rate model; the group goes when
    16 D < (((lambda_q4 k >> 1) bits) >> 4) << 2 (15 - bitDepth - log2n).  -> {(group row, group column): (D, bits, threshold, dropped)} of the groups
    that hold a level.  Plain integers, one group after the other."""
    n = 1 << log2n
    lam = (int(lambda_q4) * int(k)) >> 1
    shift = 2 * (15 - bit_depth - log2n)
    out = {}
    for gy in range(0, n, 4):
        for gx in range(0, n, 4):
            d, bits, any_level = 0, R_SB, False
            for y in range(gy, gy + 4):
                for x in range(gx, gx + 4):
                    a = int(lvl[y][x])
                    if a == 0:
                        continue
                    any_level = True
                    c, r = int(coef[y][x]), int(deq[y][x])
                    d += r * (2 * c - r)
                    bits += level_rate(abs(a))
            if any_level:
                threshold = ((lam * bits) >> 4) << shift
                out[gy >> 2, gx >> 2] = (d, bits, threshold, 16 * d < threshold)
    return out


def integer_table(cur_y, ref_y, bit_depth, me_range, lambda_sad_q4, centres, mc_top=0, mc_bottom=0):
    """the 21-node integer table the program starts from: A.integer_search; in a slice (*Slices*), which that model does not state, the same
    rules walked candidate by candidate: a vertical displacement that takes the node's rows (luma, or chroma at its half-sample phase) out of the slice is
    no candidate.  centres: (n_ctu, 2) whole samples, in a slice the CLAMPED ones"""
    if not (mc_top or mc_bottom):
        return A.integer_search(cur_y, ref_y, bit_depth, me_range, lambda_sad_q4, centres)
    src, ref = np.asarray(cur_y).astype(np.int64) >> (bit_depth - 8), np.asarray(ref_y).astype(np.int64) >> (bit_depth - 8)
    h, w = src.shape
    spanx, _ = A.search_span(me_range)
    wc, hc = (w + CTU - 1) // CTU, (h + CTU - 1) // CTU
    P = 64 + me_range + spanx + 32
    refp = np.pad(ref, P, mode="edge")
    out = np.zeros((wc * hc, 21, 3), np.int32)
    for ctu in range(len(out)):
        x0, y0, (sx, sy) = ctu % wc * CTU, ctu // wc * CTU, (int(v) for v in centres[ctu])
        for nd, (nx, ny, n) in enumerate(NODES):
            out[ctu, nd] = (0, 0, -1)
            if x0 + nx + n > w or y0 + ny + n > h:
                continue
            best = None
            for dy in range(-me_range, me_range + 1):
                if not rows_inside(y0 + ny, n, 4 * (sy + dy), h, mc_top, mc_bottom):
                    continue
                for dx in range(-me_range, -me_range + spanx):
                    gy, gx = P + y0 + ny + sy + dy, P + x0 + nx + sx + dx
                    sad = int(np.abs(src[y0 + ny:y0 + ny + n, x0 + nx:x0 + nx + n] - refp[gy:gy + n, gx:gx + n]).sum())
                    cost = (sad << (4 + bit_depth - 8)) + lambda_sad_q4 * (A.mvd_bits(4 * dx) + A.mvd_bits(4 * dy))
                    if best is None or cost < best[2]:
                        best = (4 * (sx + dx), 4 * (sy + dy), cost)
            if best is not None:
                out[ctu, nd] = best
    return out


class Result:
    """cu: (h / 8, w / 8) CU_DTYPE; coef, rec: three planes each; est: 1/16 bit; ctus: per CTU a dict for diagnosis (see analyse)"""

    def __init__(self, w, h):
        self.cu = np.zeros((h // 8, w // 8), CU_DTYPE)
        self.coef = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
        self.rec = [np.zeros((h, w), np.int64), np.zeros((h // 2, w // 2), np.int64), np.zeros((h // 2, w // 2), np.int64)]
        self.est = 0
        self.ctus = []


def analyse(src, refs, tables, bit_depth, qp, qp_c, lambda_sad_q4, lambda_q4, me_range, centres=None, rdo_zero=0, mc_top=0, mc_bottom=0, cov=None, rdo_cg=0, sign_hide=0):
    """src: (Y, Cb, Cr) of the coded size; refs: one (P picture) or two (B picture: list 0, list 1) such triples, unpadded: reads beyond the picture
    are clamped to it; tables: per reference the (n_ctu, 21, 3) integer-search dump (A.integer_search); centres: per reference None or (n_ctu, 2)
    whole samples, as they were given to the search.

    Result.ctus[i]: {"leaves": [node ...], "node_cost": {node: integer-vector cost}, "tree": (whole / split pairs),
    "rounds": {(node, list, round): ([9 costs or None], winner, [9 rows-admissible flags])}, "mv": {node: [mv per list]},
    "keys": {node: [3 keys]}, "mode": {node: 0 / 1 / 2}, "tus": {(node, plane): (jz, jc, zeroed)},
    "groups": {(node, plane): {(group row, group column): (D, bits, threshold, dropped)}} (rdo_cg > 0: group_zero_out)}"""
    cov = cov if cov is not None else collections.Counter()
    sp = [np.asarray(p).astype(np.int64) for p in src]
    rp = [[np.asarray(p).astype(np.int64) for p in r] for r in refs]
    h, w = sp[0].shape
    bd, lam, maxv = bit_depth, lambda_sad_q4, (1 << bit_depth) - 1
    wc, hc = (w + CTU - 1) // CTU, (h + CTU - 1) // CTU
    slice_ = bool(mc_top or mc_bottom)
    cen = [np.zeros((wc * hc, 2), np.int64) if c is None else np.asarray(c).astype(np.int64).reshape(wc * hc, 2) for c in (centres or [None] * len(refs))]
    out = Result(w, h)

    def luma_cost(l, gx, gy, n, mv, centre):
        pred = R.weighted_default([R.mc_luma(rp[l][0], gx, gy, n, mv, bd)], bd)
        return (satd(sp[0][gy:gy + n, gx:gx + n] - pred) << 4) + lam * mv_bits(mv, centre)

    def refine(info, nd, l, gx, gy, n, mv, cost, centre):
        for rnd, step in enumerate((2, 1)):
            cands = [mv] + [(mv[0] + dx * step, mv[1] + dy * step) for dx, dy in RING]
            ok = [True] + [not slice_ or rows_inside(gy, n, c[1], h, mc_top, mc_bottom) for c in cands[1:]]
            price = [cost] + [luma_cost(l, gx, gy, n, c, centre) for c in cands[1:]]
            best = None
            for k in range(9):                                   # a plain walk: a later candidate must be strictly cheaper
                if ok[k] and (best is None or price[k] < price[best]):
                    best = k
            info["rounds"][nd, l, rnd] = (price, best, ok)
            cov["half" if rnd == 0 else "quarter", best] += 1
            tied = [k for k in range(9) if ok[k] and price[k] == price[best]]
            if len(tied) > 1:
                cov["ring tie"] += 1
                if 0 not in tied:                                # between ring positions alone: the centre is not among them
                    cov["ring tie", "ring only"] += 1
            if min(price) < price[best]:
                cov["slice removed the winner"] += 1
            mv, cost = cands[best], price[best]
        return mv, cost

    for ctu in range(wc * hc):
        x0, y0 = ctu % wc * CTU, ctu // wc * CTU
        centre = []
        for l in range(len(refs)):
            sx, sy = int(cen[l][ctu, 0]), int(cen[l][ctu, 1])
            centre.append((sx, clamp_centre_y(sy, y0, me_range, h, mc_top, mc_bottom) if slice_ else sy))
        valid = [int(tables[0][ctu, nd, 2]) >= 0 for nd in range(21)]
        info = {"leaves": [], "node_cost": {}, "rounds": {}, "mv": {}, "keys": {}, "mode": {}, "tus": {}, "groups": {}}
        # ---- node cost at the integer vector
        c0 = {}
        for nd, (nx, ny, n) in enumerate(NODES):
            if not valid[nd]:
                cov["invalid node"] += 1
                continue
            mv = (int(tables[0][ctu, nd, 0]), int(tables[0][ctu, nd, 1]))
            c0[nd] = luma_cost(0, x0 + nx, y0 + ny, n, mv, centre[0])
        info["node_cost"] = dict(c0)
        # ---- the tree, bottom-up
        use16, j16, pairs = [False] * 4, [0] * 4, []
        for q in range(4):
            split = 2 * lam + sum(c0[k] + 4 * lam for k in range(5 + 4 * q, 9 + 4 * q) if valid[k])
            j16[q] = split
            if valid[1 + q]:
                whole = c0[1 + q] + 4 * lam
                use16[q] = whole <= split
                pairs.append((whole, split))
                if whole == split:
                    cov["whole == split"] += 1
                if use16[q]:
                    j16[q] = whole
        use32 = False
        if valid[0]:
            whole, split = c0[0] + 4 * lam, 2 * lam + sum(j16)
            use32 = whole <= split
            pairs.append((whole, split))
            if whole == split:
                cov["whole == split"] += 1
        info["tree"] = pairs
        for nd in range(21):
            leaf = valid[nd] and (use32 if nd == 0 else (not use32 and use16[nd - 1]) if nd < 5 else (not use32 and not use16[(nd - 5) >> 2]))
            if leaf:
                info["leaves"].append(nd)
                cov["leaf", NODES[nd][2]] += 1
        # ---- the chosen CUs
        for nd in info["leaves"]:
            nx, ny, n = NODES[nd]
            gx, gy = x0 + nx, y0 + ny
            mv0, cost0 = refine(info, nd, 0, gx, gy, n, (int(tables[0][ctu, nd, 0]), int(tables[0][ctu, nd, 1])), c0[nd], centre[0])
            mvs, mode = [mv0], L0
            if len(refs) == 2:
                mv1 = (int(tables[1][ctu, nd, 0]), int(tables[1][ctu, nd, 1]))
                mv1, cost1 = refine(info, nd, 1, gx, gy, n, mv1, luma_cost(1, gx, gy, n, mv1, centre[1]), centre[1])
                both = R.weighted_default([R.mc_luma(rp[0][0], gx, gy, n, mv0, bd), R.mc_luma(rp[1][0], gx, gy, n, mv1, bd)], bd)
                keys = [cost0 + 2 * lam, cost1 + 2 * lam,
                        (satd(sp[0][gy:gy + n, gx:gx + n] - both) << 4) + lam * (mv_bits(mv0, centre[0]) + mv_bits(mv1, centre[1])) + lam]
                mode = keys.index(min(keys))                     # list 0, list 1, both: the first of equal keys
                if keys.count(min(keys)) > 1:
                    cov["B key tie"] += 1
                    cov["B key tie", tuple(m for m in (L0, L1, BI) if keys[m] == min(keys))] += 1      # which keys are equal
                cov["B mode", mode] += 1
                mvs = [mv0, mv1]
                info["keys"][nd] = keys
            info["mv"][nd], info["mode"][nd] = mvs, mode
            used = [l for l in range(len(refs)) if mode == BI or mode == l]
            flags, cu_bits = F_INTER, R_CU
            for c in range(3):
                sh = 1 if c else 0
                px, py, m, q = gx >> sh, gy >> sh, n >> sh, qp_c if c else qp
                mc = R.mc_chroma if c else R.mc_luma
                pred = R.weighted_default([mc(rp[l][c], px, py, m, mvs[l], bd) for l in used], bd)
                blk = sp[c][py:py + m, px:px + m]
                log2m = m.bit_length() - 1
                coef = K3.forward((blk - pred)[None], log2m, bd)
                lvl = K3.quantise(coef, log2m, q, bd, False)
                deq = K3.scale(lvl, log2m, q, bd)
                coef, lvl, deq = coef[0], lvl[0], deq[0]
                thinned = False
                if rdo_cg > 0 and lvl.any():                      # the group drop: before the cbf, the TU zero-out and the estimate
                    groups = info["groups"][nd, c] = group_zero_out(coef, lvl, deq, log2m, bd, lambda_q4, rdo_cg)
                    where = ("luma" if c == 0 else "chroma", m)
                    for (gr, gc), (dist, gbits, thr, drop) in groups.items():
                        cov["group", where, "dropped" if drop else "kept"] += 1
                        if 16 * dist == thr:
                            cov["group equality"] += 1
                        if drop:
                            lvl[4 * gr:4 * gr + 4, 4 * gc:4 * gc + 4] = 0
                            deq[4 * gr:4 * gr + 4, 4 * gc:4 * gc + 4] = 0
                            thinned = True
                    if not lvl.any():
                        cov["group drop emptied a TU"] += 1
                if sign_hide and lvl.any():                       # sign data hiding: after the group decisions, before the TU zero-out; inter TUs scan diagonally
                    qq = q + 6 * (bd - 8)
                    before = lvl.copy()
                    for gr in range(0, m, 4):
                        for gc in range(0, m, 4):
                            SDH.hide_group(lvl[gr:gr + 4, gc:gc + 4], coef[gr:gr + 4, gc:gc + 4], 0, K3.QUANT_SCALE[qq % 6], 14 + qq // 6 + (15 - bd - log2m))
                            if not np.array_equal(before[gr:gr + 4, gc:gc + 4], lvl[gr:gr + 4, gc:gc + 4]):
                                cov["sign hiding adjusted a group"] += 1
                                if thinned:
                                    cov["sign hiding adjusted a group", "in a TU that lost a group"] += 1
                    deq = K3.scale(lvl, log2m, q, bd)
                res = K3.inverse(deq[None], log2m, bd)[0] if lvl.any() else np.zeros_like(lvl)
                if rdo_zero and lvl.any():
                    dz, dc = blk - pred, blk - np.clip(pred + res, 0, maxv)
                    jz = int((dz * dz).sum()) << 4
                    jc = (int((dc * dc).sum()) << 4) + ((lambda_q4 * (sub_block_bits(lvl) + R_TU)) >> 4)
                    zero = jz <= jc
                    info["tus"][nd, c] = (jz, jc, zero)
                    cov["zero-out", "zeroed" if zero else "kept"] += 1
                    if jz == jc:
                        cov["zero-out tie"] += 1
                    if zero:
                        lvl, res = np.zeros_like(lvl), np.zeros_like(res)
                        if thinned:
                            cov["group drop thinned, zero-out removed"] += 1
                if lvl.any():
                    flags |= F_CBF[c]
                    cu_bits += R_TU + sub_block_bits(lvl)
                out.coef[c][py:py + m, px:px + m] = lvl
                out.rec[c][py:py + m, px:px + m] = np.clip(pred + res, 0, maxv)
            out.est += cu_bits
            r = out.cu[gy >> 3:(gy + n) >> 3, gx >> 3:(gx + n) >> 3]
            r["log2_size"], r["chroma_mode"], r["qp"] = n.bit_length() - 1, 1, qp
            r["intra_mode"] = (1, 0, 0, 0)
            r["mvx"], r["mvy"] = mv0 if mode != L1 else (0, 0)                 # a list the CU does not use reports a zero vector
            if len(refs) == 2:
                x1, y1 = mvs[1] if mode != L0 else (0, 0)
                r["intra_mode"] = (x1 & 255, (x1 >> 8) & 255, y1 & 255, (y1 >> 8) & 255)
                flags |= (F_L1 if mode != L0 else 0) | (F_NOL0 if mode == L1 else 0)
            r["flags"] = flags
        out.ctus.append(info)
    return out
