"""A third statement of the encoder-side decisions whose inputs and outputs leave the stage entry points: the 1/4-size pictures and the search
centres made from them, the integer motion search of every quadtree node (the `me_dump` table) and the SAO parameters of every CTU.

Written from the documents alone: DESIGN.md §6 ("Decision rules, in words"), the header comment of hevc_amd/csrc/kernels/inter.h, the comments of
include/mihevc.h and H.265 8.7.3 for the SAO edge categories.  Not from oracle/hevc_oracle.c and not from the kernel bodies, which are one
author's two statements of the same rules and share their structure (a table of 8x8 SADs, a packed (cost << 16 | position) key, a walk from the
rounded mean towards zero).  Everything here is brute force instead: whole windows by numpy, every candidate offset priced, the first minimum taken.

Imports: numpy and the standard library only (tests/test_syntax_independent.py checks it)."""
import numpy as np

CTU = 32
PRE_RANGE = 14                       # the pre-search covers +-14 low-resolution samples = +-56 luma samples
MAX_CENTRE = 64                      # what this model pads for; a session's centres stay within +-56
MAX_RANGE = 64                       # include/mihevc.h: me_range <= 64

# include/mihevc.h, mihevc_sao_ctu: index 0 = luma, 1 = chroma (Cb and Cr share type and class); band_pos and offset per component Y, Cb, Cr
SAO_DTYPE = np.dtype([("type", "u1", (2,)), ("eo_class", "u1", (2,)), ("band_pos", "u1", (3,)), ("offset", "i1", (3, 4)), ("pad", "u1")])
SAO_OFF, SAO_BAND, SAO_EDGE = 0, 1, 2


def n_ctus(w, h):
    return ((w + CTU - 1) // CTU) * ((h + CTU - 1) // CTU)


# ================================================================ quadtree nodes of a CTU, in the order of the dump
def node_geometry():
    """(x, y, size) of the 21 nodes inside their CTU: the 32x32, then the four 16x16 in z-order (top left, top right, bottom left, bottom right),
    then the 8x8 of the first 16x16 in z-order, of the second, ..."""
    out = [(0, 0, 32)]
    quads = [(0, 0), (1, 0), (0, 1), (1, 1)]
    out += [(16 * qx, 16 * qy, 16) for qx, qy in quads]
    out += [(16 * qx + 8 * sx, 16 * qy + 8 * sy, 8) for qx, qy in quads for sx, sy in quads]
    return out


NODES = node_geometry()


# ================================================================ a. 1/4-size pictures and search centres
def lowres(luma, bit_depth):
    """the rounded mean of every 4x4 luma block reduced to 8 bits, in one rounding: (sum + 8 * 2^(bd - 8)) >> (4 + bd - 8), saturated at 255 (at 10 bit
    a mean of 1022 or more would round to 256)"""
    p = np.asarray(luma).astype(np.int64)
    lh, lw = p.shape[0] >> 2, p.shape[1] >> 2
    sh = bit_depth - 8
    s = p[:4 * lh, :4 * lw].reshape(lh, 4, lw, 4).sum(axis=(1, 3))
    return np.minimum((s + (8 << sh)) >> (4 + sh), 255)


def pre_search(lsrc, lref):
    """per CTU (raster order) the search centre (sx, sy) in whole luma samples: the CTU's 8x8 low-resolution block (smaller at the right and bottom
    edge of the low-resolution picture) against every displacement of +-14 with reads clamped to the low-resolution picture; cost = 4 SAD + |dx| + |dy|,
    the raster-first minimum wins (dy-major); the centre moves there only if that SAD, doubled, is still below the SAD at zero displacement"""
    lsrc, lref = np.asarray(lsrc).astype(np.int64), np.asarray(lref).astype(np.int64)
    lh, lw = lsrc.shape
    R = PRE_RANGE
    ref = np.pad(lref, R, mode="edge")                                      # clamped reads
    d = np.arange(-R, R + 1)
    pull = np.abs(d)[:, None] + np.abs(d)[None, :]                          # [dy, dx]
    out = []
    for y0 in range(0, lh, 8):
        for x0 in range(0, lw, 8):
            blk = lsrc[y0:y0 + 8, x0:x0 + 8]
            bh, bw = blk.shape
            sad = np.empty((2 * R + 1, 2 * R + 1), np.int64)
            for iy in range(2 * R + 1):
                for ix in range(2 * R + 1):
                    sad[iy, ix] = np.abs(blk - ref[y0 + iy:y0 + iy + bh, x0 + ix:x0 + ix + bw]).sum()
            cost = 4 * sad + pull
            iy, ix = np.unravel_index(np.argmin(cost), cost.shape)            # argmin: the first minimum of the flattened (dy-major) array
            if 2 * sad[iy, ix] < sad[R, R]:
                out.append((4 * (ix - R), 4 * (iy - R)))
            else:
                out.append((0, 0))
    return np.array(out, np.int16).reshape(-1, 2)


# ================================================================ b. integer search, brute force
def mvd_bits(d):
    """bits(0) = 1, bits(+-1) = 3, otherwise 3 + 2 floor(log2 |d|); d in quarter samples"""
    d = abs(int(d))
    return 1 if d == 0 else 3 + 2 * (d.bit_length() - 1)


def search_span(R):
    """(spanx, spany): dy in [-R, R]; dx in [-R, -R + spanx - 1] with spanx = 2R + 1 rounded UP to a multiple of 4"""
    return (2 * R + 1 + 3) // 4 * 4, 2 * R + 1


def integer_search(src_y, ref_y, bit_depth, me_range, lambda_sad_q4, centres=None):
    """the dump: (n_ctu, 21, 3) int32 of (mvx, mvy, cost), vectors in quarter samples INCLUDING the centre; a node that is not wholly inside the
    picture reports (0, 0, -1).  src_y, ref_y: luma planes of the coded size; the reference is read at coordinates clamped to the picture.
    centres: None or per CTU (sx, sy) in whole samples."""
    src, ref = np.asarray(src_y).astype(np.int64), np.asarray(ref_y).astype(np.int64)
    h, w = src.shape
    assert ref.shape == src.shape and 1 <= me_range <= MAX_RANGE
    R, sh = me_range, bit_depth - 8
    spanx, spany = search_span(R)
    src, ref = src >> sh, ref >> sh                                          # Main10: both pictures lose their low bits BEFORE the SAD
    wc, hc = (w + CTU - 1) // CTU, (h + CTU - 1) // CTU
    srcp = np.zeros((hc * CTU, wc * CTU), np.int64)
    srcp[:h, :w] = src
    P = MAX_CENTRE + R + spanx                                               # room for every candidate of every CTU
    refp = np.pad(ref, ((P, P + CTU), (P, P + CTU)), mode="edge")            # clamping to the picture = replicating its edge
    cen = np.zeros((wc * hc, 2), np.int64) if centres is None else np.asarray(centres).astype(np.int64).reshape(wc * hc, 2)
    assert np.abs(cen).max(initial=0) <= MAX_CENTRE
    dxs, dys = np.arange(-R, -R + spanx), np.arange(-R, R + 1)
    bits = np.array([mvd_bits(4 * dy) for dy in dys], np.int64)[:, None] + np.array([mvd_bits(4 * dx) for dx in dxs], np.int64)[None, :]
    out = np.zeros((wc * hc, 21, 3), np.int32)
    for ctu in range(wc * hc):
        x0, y0 = ctu % wc * CTU, ctu // wc * CTU
        sx, sy = int(cen[ctu, 0]), int(cen[ctu, 1])
        tile = srcp[y0:y0 + CTU, x0:x0 + CTU]
        win = refp[P + y0 + sy - R:P + y0 + sy + R + CTU, P + x0 + sx - R:P + x0 + sx - R + spanx - 1 + CTU]
        views = np.lib.stride_tricks.sliding_window_view(win, (CTU, CTU))    # [dy, dx, y, x]
        assert views.shape[:2] == (spany, spanx)
        diff = np.abs(views - tile)
        for node, (nx, ny, n) in enumerate(NODES):
            if x0 + nx + n > w or y0 + ny + n > h:
                out[ctu, node] = (0, 0, -1)
                continue
            sad = diff[:, :, ny:ny + n, nx:nx + n].sum(axis=(2, 3))
            cost = (sad << (4 + sh)) + lambda_sad_q4 * bits
            iy, ix = np.unravel_index(np.argmin(cost), cost.shape)            # ties: the smaller raster position, dy-major
            out[ctu, node] = (4 * (sx + int(dxs[ix])), 4 * (sy + int(dys[iy])), int(cost[iy, ix]))
    return out


# ================================================================ c. SAO
EO_NEIGHBOURS = (((-1, 0), (1, 0)), ((0, -1), (0, 1)), ((-1, -1), (1, 1)), ((1, -1), (-1, 1)))     # 8.7.3.2 Table 8-12: (hPos, vPos) of a and b per class


def edge_categories(plane):
    """(4, H, W): per edge class the category 0..4 of every sample of a deblocked plane.  8.7.3.2: edgeIdx = 2 + sign(c - a) + sign(c - b); edgeIdx 0, 1, 2
    are remapped to 1, 2, 0.  So 1 = a local minimum, 2 = an edge with one equal neighbour from below, 3 = the same from above, 4 = a local maximum, 0 = none.
    A sample with a neighbour outside the picture is category 0."""
    p = np.asarray(plane).astype(np.int64)
    h, w = p.shape
    big = np.pad(p, 1, mode="edge")
    inside = np.pad(np.ones((h, w), bool), 1, constant_values=False)
    out = np.zeros((4, h, w), np.int64)
    for cls, nbs in enumerate(EO_NEIGHBOURS):
        idx = np.full((h, w), 2, np.int64)
        ok = np.ones((h, w), bool)
        for dx, dy in nbs:
            idx += np.sign(p - big[1 + dy:1 + dy + h, 1 + dx:1 + dx + w])
            ok &= inside[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        cat = np.where(idx == 2, 0, np.where(idx < 2, idx + 1, idx))
        out[cls] = np.where(ok, cat, 0)
    return out


def ctb_statistics(src, dbk, cats, bit_depth, x0, y0, size):
    """count and sum of (source - deblocked) per edge class and category, and per band (deblocked sample >> (bd - 5)), over the CTB's samples inside the plane"""
    d = (np.asarray(src).astype(np.int64) - np.asarray(dbk).astype(np.int64))[y0:y0 + size, x0:x0 + size].ravel()
    band = (np.asarray(dbk).astype(np.int64)[y0:y0 + size, x0:x0 + size] >> (bit_depth - 5)).ravel()
    eo_n, eo_s = np.zeros((4, 5), np.int64), np.zeros((4, 5), np.int64)
    for cls in range(4):
        k = cats[cls, y0:y0 + size, x0:x0 + size].ravel()
        eo_n[cls] = np.bincount(k, minlength=5)
        eo_s[cls] = np.bincount(k, weights=d, minlength=5).astype(np.int64)
    return eo_n, eo_s, np.bincount(band, minlength=32), np.bincount(band, weights=d, minlength=32).astype(np.int64)


def max_offset(bit_depth):
    return (1 << (min(bit_depth, 10) - 5)) - 1


def best_offset(n, s, sign, lambda_q4, band, maxoff):
    """(offset, cost): the argmin over the permitted offsets of (n o^2 - 2 o s) 16 + lambda rate(o), ties to the smaller magnitude.  sign +1: o >= 0
    (edge categories 1, 2), -1: o <= 0 (categories 3, 4), 0: any (bands).  rate(0) = 1; rate(o) = min(|o| + 1, maxoff) bins, plus the sign bit of a band
    offset.  n = 0: offset 0 at the cost of its one bin."""
    if n == 0:
        return 0, lambda_q4
    cand = [o for o in range(-maxoff, maxoff + 1) if (sign >= 0 or o <= 0) and (sign <= 0 or o >= 0)]
    cand.sort(key=abs)                                                       # stable: -o before +o, which never tie unless s = 0, where 0 wins
    best = None
    for o in cand:
        rate = 1 if o == 0 else min(abs(o) + 1, maxoff) + (1 if band else 0)
        c = (int(n) * o * o - 2 * o * int(s)) * 16 + lambda_q4 * rate
        if best is None or c < best[1]:
            best = (o, c)
    return best


def ctb_candidates(eo_n, eo_s, bo_n, bo_s, lambda_q4, bit_depth):
    """the six candidates of one CTB of one colour component in their tie order — off, band, edge class 0, 1, 2, 3 — as (type, class, band position,
    offsets[4], cost).  Signalling: off 0 bits, band 7 (type 2 + position 5), edge 4 (type 2 + class 2), each times lambda."""
    maxoff = max_offset(bit_depth)
    out = [(SAO_OFF, 0, 0, (0, 0, 0, 0), 0)]
    per_band = [best_offset(bo_n[b], bo_s[b], 0, lambda_q4, True, maxoff) for b in range(32)]
    pos_cost = [sum(per_band[p + i][1] for i in range(4)) for p in range(29)]
    p = pos_cost.index(min(pos_cost))                                        # ties: the lowest position
    out.append((SAO_BAND, 0, p, tuple(per_band[p + i][0] for i in range(4)), pos_cost[p] + 7 * lambda_q4))
    for cls in range(4):
        offs = [best_offset(eo_n[cls][k], eo_s[cls][k], 1 if k <= 2 else -1, lambda_q4, False, maxoff) for k in range(1, 5)]
        out.append((SAO_EDGE, cls, 0, tuple(o for o, _ in offs), sum(c for _, c in offs) + 4 * lambda_q4))
    return out


def sao_parameters(src, dbk, bit_depth, lambda_q4, detail=None):
    """src, dbk: (Y, Cb, Cr) planes of the coded size, source and deblocked.  -> one SAO_DTYPE record per CTU in raster order.  Luma takes the cheapest of
    its six candidates; Cb and Cr share the choice: the candidate whose Cb cost + Cr cost is smallest (each with its own offsets and band position).  The first
    in the order off, band, class 0..3 wins ties.  Fields the chosen type does not use are 0.  detail: a list that receives per CTU the three candidate lists."""
    h, w = np.asarray(src[0]).shape
    wc, hc = (w + CTU - 1) // CTU, (h + CTU - 1) // CTU
    cats = [edge_categories(p) for p in dbk]
    out = np.zeros(wc * hc, SAO_DTYPE)
    for ctu in range(wc * hc):
        cx, cy = ctu % wc, ctu // wc
        cand = []
        for c in range(3):
            size = CTU if c == 0 else CTU // 2
            cand.append(ctb_candidates(*ctb_statistics(src[c], dbk[c], cats[c], bit_depth, cx * size, cy * size, size), lambda_q4, bit_depth))
        if detail is not None:
            detail.append(cand)
        luma_cost = [k[4] for k in cand[0]]
        chroma_cost = [a[4] + b[4] for a, b in zip(cand[1], cand[2])]
        bl, bc = luma_cost.index(min(luma_cost)), chroma_cost.index(min(chroma_cost))
        o = out[ctu]
        o["type"][0], o["eo_class"][0], o["band_pos"][0] = cand[0][bl][:3]
        o["offset"][0] = cand[0][bl][3]
        o["type"][1], o["eo_class"][1] = cand[1][bc][:2]
        o["band_pos"][1], o["band_pos"][2] = cand[1][bc][2], cand[2][bc][2]
        o["offset"][1], o["offset"][2] = cand[1][bc][3], cand[2][bc][3]
    return out
