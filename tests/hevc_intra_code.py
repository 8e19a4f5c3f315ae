"""A third statement of the intra CODE stage (every IDR picture), the NxN trial on top of it (`intra_nxn`) and the intra second pass of P pictures
(`intra_in_p`): what `mihevc_k_intra_frame` and `mihevc_k_inter_frame` leave behind — CU records, levels, the pre-deblock reconstruction and the
picture's rate estimate — and the costs J that decide between 2Nx2N and NxN and between the inter and the intra version of a CTU.

Written from the documents alone: DESIGN.md §6 ("Decision rules of the intra code stage, the NxN trial and the intra second pass, in words"), the
comments of include/mihevc.h and H.265 6.4.1 / 8.4.2 / 8.4.4.2 / 8.6.  Not from hevc_amd/csrc/kernels/intra.h and not from oracle/hevc_oracle.c, which
are one author's two statements of the same rules and share their structure (packed (cost << 6 | mode) keys, a parked 2Nx2N result that is restored
when NxN loses, modular correction of the estimate).  Everything here is brute force instead: whole blocks, every candidate priced into a list and
the first minimum taken, both variants of a CU computed side by side and one of them picked, a tried CTU coded on a copy of the picture.

Imports: numpy, the standard library, tests/hevc_recon.py (8.4.4.2), tests/transform_ref.py (K3), tests/sdh_ref.py (sign data hiding),
tests/hevc_intra_plan.py (the plan, the candidate list of 8.4.2, the rate of a block's levels), tests/hevc_inter_cu.py (the P picture before the
second pass) and tests/hevc_analysis.py (geometry, the pre-search) (tests/test_syntax_independent.py checks it)."""
import collections

import numpy as np

from tests import hevc_analysis as A
from tests import hevc_inter_cu as HI
from tests import hevc_intra_plan as P
from tests import hevc_recon as R
from tests import sdh_ref as SDH
from tests import transform_ref as K3

CTU = 32
NODES = A.NODES
CU_DTYPE = HI.CU_DTYPE
F_INTER, F_CBF, F_NXN = 1, (2, 4, 8), 16
R_INTRA_CU = 128                                   # 1/16 bit: the header of an intra CU in the rate estimate
DC = 1


def mode_of_record(r, x, y):
    """the luma mode a neighbouring PU answers with (8.4.2): the record of the CU that holds luma sample (x, y)"""
    if int(r["flags"]) & F_INTER:
        return DC, "an inter record"
    if int(r["flags"]) & F_NXN:
        return int(r["intra_mode"][((y >> 2) & 1) * 2 + ((x >> 2) & 1)]), "a PU of an NxN CU"
    return int(r["intra_mode"][0]), "a 2Nx2N CU"


def hadamard_ac(tile):
    """activity of one 8x8 source tile: sum |H s H^T| without the DC coefficient, (sum + 2) >> 2"""
    c = np.abs(HI.H8 @ np.asarray(tile, np.int64) @ HI.H8.T)
    return (int(c.sum()) - int(c[0, 0]) + 2) >> 2


def schedule(cand):
    """cand: (rows, columns) of booleans -> the same shape of 0 (round 0), 1 (round 1), -1 (a candidate never tried) and -2 (no candidate)"""
    cand = np.asarray(cand, bool)
    hc, wc = cand.shape
    near = ((-1, 0), (-1, -1), (0, -1), (1, -1))     # left, top-left, top, top-right as (dx, dy)

    def is_cand(x, y):
        return 0 <= x < wc and 0 <= y < hc and bool(cand[y, x])
    first = np.zeros(cand.shape, bool)
    for y in range(hc):
        for x in range(wc):
            first[y, x] = cand[y, x] and not any(is_cand(x + dx, y + dy) for dx, dy in near)
    out = np.full(cand.shape, -2)
    for y in range(hc):
        for x in range(wc):
            if not cand[y, x]:
                continue
            if first[y, x]:
                out[y, x] = 0
            elif all(first[y + dy, x + dx] for dx, dy in near if is_cand(x + dx, y + dy)):
                out[y, x] = 1
            else:
                out[y, x] = -1
    return out


class State:
    """a picture while it is coded: the pre-deblock reconstruction, the CU records, the levels"""

    def __init__(self, w, h, pic=None, cu=None, coef=None):
        self.pic = [np.array(p, np.int64) for p in pic] if pic is not None else [np.zeros((h, w), np.int64), np.zeros((h // 2, w // 2), np.int64), np.zeros((h // 2, w // 2), np.int64)]
        self.cu = np.array(cu, CU_DTYPE) if cu is not None else np.zeros((h // 8, w // 8), CU_DTYPE)
        self.coef = [np.array(c, np.int16) for c in coef] if coef is not None else [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]

    def copy(self):
        return State(0, 0, self.pic, self.cu, self.coef)


class Result:
    """cu, coef[3], rec[3], est as the stage entries return them; for diagnosis: cus = {(x, y): the CU's dict} (sse, bits per plane, cand, j, and for an NxN
    trial "nxn": per-PU cost tables, modes, j), ctus = {ctu: dict} (j_ctu, est, and in a P picture cost / act / tiles / jinter / round / replaced)"""

    def __init__(self, st, est, cus, ctus, cov):
        self.cu, self.coef, self.rec, self.est, self.cus, self.ctus, self.cov = st.cu, st.coef, st.pic, est, cus, ctus, cov

    def same(self, o):
        """two results of the model are the same outputs"""
        return (self.cu.tobytes() == o.cu.tobytes() and self.est == o.est and all(np.array_equal(a, b) for a, b in zip(self.coef, o.coef)) and
                all(np.array_equal(a, b) for a, b in zip(self.rec, o.rec)))


class IntraCodeModel:
    def __init__(self, src, prm, cov=None, list_from_plan=False):
        """src: (Y, Cb, Cr) of the coded size; prm: anything with qp, qp_c, bit_depth, lambda_sad_q4, lambda_q4, tile_cols, tile_rows, intra_nxn (and
        sign_hide).  list_from_plan: a switch for the binding test — the 2Nx2N CUs are priced with the PLAN's candidate list in place of the code stage's own"""
        self.s = [np.asarray(p).astype(np.int64) for p in src]
        self.h, self.w = self.s[0].shape
        self.bd, self.qp, self.qp_c = int(prm.bit_depth), int(prm.qp), int(prm.qp_c)
        self.lam, self.lam_sad = int(prm.lambda_q4), int(prm.lambda_sad_q4)
        self.nxn, self.sign_hide = int(prm.intra_nxn), int(getattr(prm, "sign_hide", 0))
        self.wc, self.hc = (self.w + CTU - 1) // CTU, (self.h + CTU - 1) // CTU
        self.col_bd, self.row_bd = P.tile_bounds(self.wc, max(int(prm.tile_cols), 1)), P.tile_bounds(self.hc, max(int(prm.tile_rows), 1))
        self.cov = cov if cov is not None else collections.Counter()
        self.list_from_plan = list_from_plan
        self.maxv = (1 << self.bd) - 1

    # ---------------------------------------------------------------- geometry
    def tile_box(self, lx, ly):
        """luma bounds (x_lo, x_hi, y_lo, y_hi) of the tile that holds luma sample (lx, ly)"""
        cx, cy = lx >> 5, ly >> 5
        i = max(k for k in range(len(self.col_bd) - 1) if self.col_bd[k] <= cx)
        j = max(k for k in range(len(self.row_bd) - 1) if self.row_bd[k] <= cy)
        return self.col_bd[i] * CTU, self.col_bd[i + 1] * CTU, self.row_bd[j] * CTU, self.row_bd[j + 1] * CTU

    def address(self, lx, ly):
        """z-scan address of the 4x4 unit at luma (lx, ly): CTBs in raster order, z-scan inside the CTB (6.5.2; inside one tile the order of 6.4.1)"""
        return ((np.asarray(ly) >> 5) * self.wc + (np.asarray(lx) >> 5)) * 64 + P.z_index(np.asarray(lx) & 31, np.asarray(ly) & 31)

    def references(self, pic, c, x, y, n, zx, zy):
        """-> (the 4n + 1 substituted reference samples of the n x n block at (x, y) of plane c, read from `pic`; the availability of each).  (zx, zy): the luma
        position of the block whose z-scan address decides what counts as decoded: the CU's, or a luma PU's own"""
        sh = 1 if c else 0
        k = np.arange(2 * n)
        xs = np.concatenate([np.full(2 * n, x - 1), [x - 1], x + k])
        ys = np.concatenate([y + 2 * n - 1 - k, [y - 1], np.full(2 * n, y - 1)])
        lx, ly = xs << sh, ys << sh
        x_lo, x_hi, y_lo, y_hi = self.tile_box(zx, zy)
        inside = (lx >= 0) & (ly >= 0) & (lx < self.w) & (ly < self.h) & (lx >= x_lo) & (lx < x_hi) & (ly >= y_lo) & (ly < y_hi)
        avail = inside & (self.address(np.clip(lx, 0, self.w - 1), np.clip(ly, 0, self.h - 1)) < self.address(zx, zy))
        plane = pic[c]
        raw = np.where(avail, plane[np.clip(ys, 0, plane.shape[0] - 1), np.clip(xs, 0, plane.shape[1] - 1)], 0)
        return R.substitute(raw, avail, self.bd), avail

    # ---------------------------------------------------------------- one transform block
    def block(self, src, pred, log2n, qp, dst, scan):
        """-> (levels, reconstruction) of one transform block: K3 with intra rounding, sign data hiding per 4x4 group when on, clip(prediction + residual)"""
        n = 1 << log2n
        coef = K3.forward((src - pred)[None], log2n, self.bd, dst)[0]
        lvl = np.array(K3.quantise(coef, log2n, qp, self.bd, True), np.int64)
        if self.sign_hide and lvl.any():
            q = qp + 6 * (self.bd - 8)
            before = lvl.copy()
            for gy in range(0, n, 4):
                for gx in range(0, n, 4):
                    SDH.hide_group(lvl[gy:gy + 4, gx:gx + 4], coef[gy:gy + 4, gx:gx + 4], scan, K3.QUANT_SCALE[q % 6], 14 + q // 6 + (15 - self.bd - log2n))
            self.cov["sign hiding adjusted a block"] += int(not np.array_equal(before, lvl))
        res = K3.inverse(K3.scale(lvl[None], log2n, qp, self.bd), log2n, self.bd, dst)[0] if lvl.any() else np.zeros((n, n), np.int64)
        return lvl, np.clip(pred + res, 0, self.maxv)

    # ---------------------------------------------------------------- candidate lists
    def neighbour_mode(self, st, x, y, px, py, own):
        """candIntraPredModeX of the PU at luma (px, py) from the PU that holds luma sample (x, y), which lies left of it (same row) or above it (same column).
        own: {(x >> 2, y >> 2): mode} of the PUs of the CU being tried as NxN"""
        if own is not None and (x >> 2, y >> 2) in own:
            return own[x >> 2, y >> 2], "a PU of the same CU"
        if y < py and (py & 31) == 0:
            return DC, "the CTU above"
        if x < 0 or y < 0:
            return DC, "the picture's edge"
        if x < px and (px & 31) == 0 and x < self.tile_box(px, py)[0]:
            return DC, "a tile's edge"
        m, what = mode_of_record(st.cu[y >> 3, x >> 3], x, y)
        if x < px and (px & 31) == 0:
            what = "the left CTU: " + what
        return m, what

    def cand_list(self, st, px, py, own=None):
        a, wa = self.neighbour_mode(st, px - 1, py, px, py, own)
        b, wb = self.neighbour_mode(st, px, py - 1, px, py, own)
        self.cov["list", "left", wa] += 1
        self.cov["list", "above", wb] += 1
        if own is not None:
            self.cov["PU list", "left", wa] += 1
            self.cov["PU list", "above", wb] += 1
        return P.cand_mode_list(a, b)

    def plan_list(self, plan, nd):
        """the PLAN's list of node nd (the intra plan): same-level nodes inside the CTU, DC outside"""
        x, y, n = NODES[nd]
        a = int(plan["mode"][P.NODE_AT[(x - n, y, n)]]) if x > 0 else DC
        b = int(plan["mode"][P.NODE_AT[(x, y - n, n)]]) if y > 0 else DC
        return P.cand_mode_list(a, b)

    # ---------------------------------------------------------------- one CU, both ways
    def cu_2nx2n(self, st, gx, gy, n, mode, cmode, cand):
        out = {"size": n, "mode": mode, "cmode": cmode, "cand": cand, "rec": [], "lvl": [], "bits": []}
        sse, flags = 0, 0
        for c in range(3):
            x, y, m, q, k = (gx, gy, n, self.qp, mode) if c == 0 else (gx // 2, gy // 2, n // 2, self.qp_c, cmode)
            p, _ = self.references(st.pic, c, x, y, m, gx, gy)
            if c == 0:
                p = R.filter_refs(p, m, k, self.bd, True)
            pred = R.predict_intra(p, m, k, c, self.bd)
            src = self.s[c][y:y + m, x:x + m]
            lvl, rec = self.block(src, pred, m.bit_length() - 1, q, False, SDH.scan_idx(m.bit_length() - 1, c, k))
            d = src - rec
            sse += int((d * d).sum())
            out["rec"].append(rec)
            out["lvl"].append(lvl)
            out["bits"].append(P.coefficient_bits(lvl))
            flags |= F_CBF[c] if lvl.any() else 0
        bits = 16 * P.mode_bits(cand, mode) + 16 + 24 + (32 if cmode != mode else 0) + sum(out["bits"])
        rec = np.zeros((), CU_DTYPE)
        rec["log2_size"], rec["flags"], rec["chroma_mode"], rec["qp"], rec["intra_mode"] = n.bit_length() - 1, flags, cmode, self.qp, mode
        out.update(sse=sse, total_bits=bits, j=(sse << 4) + ((self.lam * bits) >> 4), record=rec, est=R_INTRA_CU + sum(out["bits"]))
        return out

    def cu_nxn(self, st, gx, gy):
        pic = [p.copy() for p in st.pic]                # the PUs are coded in place, each seeing those before it; st itself is not touched
        own, modes, tables, lists = {}, [], [], []
        bits, sse, flags, cbf_y4, est = 16 + 24, 0, F_NXN, 0, R_INTRA_CU
        out = {"size": 8, "rec": [np.zeros((8, 8), np.int64)], "lvl": [np.zeros((8, 8), np.int64)], "bits": [0, 0, 0]}
        for k in range(4):
            ox, oy = (k & 1) * 4, (k >> 1) * 4
            bx, by = gx + ox, gy + oy
            p, avail = self.references(pic, 0, bx, by, 4, bx, by)      # availability by the PU's own address; never filtered
            if not avail.all():
                self.cov["PU with an unavailable sample", k] += 1
                if (~avail[:4]).all() and avail[4:8].all():             # (17 samples: 4 bottom-left, 4 left, the corner, 4 above, 4 top-right)
                    self.cov["PU without bottom-left", k] += 1
                if (~avail[13:]).all() and avail[9:13].all():
                    self.cov["PU without top-right", k] += 1
            cand = self.cand_list(st, bx, by, own)
            src = self.s[0][by:by + 4, bx:bx + 4]
            preds = np.stack([R.predict_intra(p, 4, m, 0, self.bd) for m in range(35)])
            cost = [(int(P.satd(src - preds[m], 4)) << 4) + self.lam_sad * P.mode_bits(cand, m) for m in range(35)]
            m = cost.index(min(cost))                                   # the lowest cost, of equal costs the lowest mode
            lvl, rec = self.block(src, preds[m], 2, self.qp, True, SDH.scan_idx(2, 0, m))
            pic[0][by:by + 4, bx:bx + 4] = rec
            own[bx >> 2, by >> 2] = m
            d = src - rec
            sse += int((d * d).sum())
            b = P.coefficient_bits(lvl)
            bits += 16 * P.mode_bits(cand, m) + b
            est += b
            out["bits"][0] += b
            if lvl.any():
                cbf_y4 |= 1 << k
                flags |= F_CBF[0]
            out["rec"][0][oy:oy + 4, ox:ox + 4], out["lvl"][0][oy:oy + 4, ox:ox + 4] = rec, lvl
            modes.append(m)
            tables.append(cost)
            lists.append(cand)
        for c in (1, 2):                                                # one 4x4 each, PU 0's mode, availability by the CU's address
            x, y = gx // 2, gy // 2
            p, _ = self.references(pic, c, x, y, 4, gx, gy)
            pred = R.predict_intra(p, 4, modes[0], c, self.bd)
            src = self.s[c][y:y + 4, x:x + 4]
            lvl, rec = self.block(src, pred, 2, self.qp_c, False, SDH.scan_idx(2, c, modes[0]))
            d = src - rec
            sse += int((d * d).sum())
            b = P.coefficient_bits(lvl)
            bits += b
            est += b
            out["bits"][c] = b
            flags |= F_CBF[c] if lvl.any() else 0
            out["rec"].append(rec)
            out["lvl"].append(lvl)
        rec = np.zeros((), CU_DTYPE)
        rec["log2_size"], rec["flags"], rec["chroma_mode"], rec["qp"], rec["intra_mode"], rec["cbf_y4"] = 3, flags, modes[0], self.qp, modes, cbf_y4
        out.update(sse=sse, total_bits=bits, j=(sse << 4) + ((self.lam * bits) >> 4), record=rec, est=est, modes=modes, tables=tables, lists=lists, mode=modes[0], cmode=modes[0])
        return out

    def code_cu(self, st, x0, y0, nd, plan):
        """codes leaf nd of the CTU at (x0, y0) into st; -> the dict of the variant that was kept"""
        nx, ny, n = NODES[nd]
        gx, gy = x0 + nx, y0 + ny
        mode, cmode = int(plan["mode"][nd]), int(plan["cmode"][nd])
        cand = self.cand_list(st, gx, gy)
        if self.list_from_plan:
            cand = self.plan_list(plan, nd)
        kept = two = self.cu_2nx2n(st, gx, gy, n, mode, cmode, cand)
        if self.nxn and n == 8:
            if two["lvl"][0].any():
                four = self.cu_nxn(st, gx, gy)
                keep = four["j"] < two["j"]                              # the 2Nx2N coding wins ties
                self.cov["nxn", "kept" if keep else "refused"] += 1
                self.cov["nxn", "tie"] += int(four["j"] == two["j"])
                if keep:
                    kept = four
                kept = dict(kept, nxn=dict(j_2nx2n=two["j"], j_nxn=four["j"], tables=four["tables"], lists=four["lists"], modes=four["modes"], kept=keep,
                                           sse=four["sse"], total_bits=four["total_bits"], sse_2nx2n=two["sse"], total_bits_2nx2n=two["total_bits"]))
            else:
                self.cov["nxn", "not tried"] += 1
                self.cov["nxn", "not tried, chroma has a level"] += int(two["lvl"][1].any() or two["lvl"][2].any())
        for c in range(3):
            sh = 1 if c else 0
            x, y, m = gx >> sh, gy >> sh, n >> sh
            st.pic[c][y:y + m, x:x + m] = kept["rec"][c]
            st.coef[c][y:y + m, x:x + m] = kept["lvl"][c]
        st.cu[gy >> 3:(gy + n) >> 3, gx >> 3:(gx + n) >> 3] = kept["record"]
        return kept

    def code_ctu(self, st, ctu, plan):
        """the leaves of the plan in decoding order, coded into st -> {"j": J_ctu, "est": the CTU's estimate, "cus": {(x, y): dict}}"""
        x0, y0 = ctu % self.wc * CTU, ctu // self.wc * CTU
        cus, est = {}, 0
        if plan["chosen"][0]:
            k = cus[x0, y0] = self.code_cu(st, x0, y0, 0, plan)
            return {"j": self.lam + k["j"], "est": k["est"], "cus": cus}
        j = self.lam
        for q in range(4):
            kids = [5 + 4 * q + b for b in range(4) if plan["chosen"][5 + 4 * q + b]]
            for nd in kids + ([1 + q] if plan["chosen"][1 + q] else []):
                k = cus[x0 + NODES[nd][0], y0 + NODES[nd][1]] = self.code_cu(st, x0, y0, nd, plan)
                j += k["j"]
                est += k["est"]
            if kids or plan["chosen"][1 + q]:
                j += self.lam
        return {"j": j, "est": est, "cus": cus}


def code_picture(src, plan, prm, picture_before=None, records_before=None, cov=None, list_from_plan=False):
    """An I picture: every CTU of the plan, in raster order (what a CTU may see of its neighbours has then been coded: 6.4.1), from an empty picture
    or from picture_before / records_before.  -> Result"""
    m = IntraCodeModel(src, prm, cov, list_from_plan)
    st = State(m.w, m.h, picture_before, records_before)
    cus, ctus, est = {}, {}, 0
    for ctu in range(m.wc * m.hc):
        info = m.code_ctu(st, ctu, plan[ctu])
        cus.update(info["cus"])
        ctus[ctu] = {"j_ctu": info["j"], "est": info["est"]}
        est += info["est"]
    return Result(st, est, cus, ctus, m.cov)


def second_pass(src, ref, prm, centres=None, cov=None, list_from_plan=False, activity_with_dc=False, planted=None):
    """A P picture with `intra_in_p`: the inter CTU program (tests/hevc_inter_cu.py), the candidate flag, the two rounds, the J comparison and the estimate.
    src, ref: (Y, Cb, Cr); centres: None or (n_ctu, 2) whole samples; activity_with_dc: a switch for the binding test; planted: {ctu: {"cost": .., "act": ..,
    "tiles": ..}} overrides of the three sums the candidate test reads (the twin in which its boundaries are planted).  -> Result; Result.inter is the model
    of the picture before the second pass"""
    cov = cov if cov is not None else collections.Counter()
    sp = [np.asarray(p).astype(np.int64) for p in src]
    rp = [np.asarray(p).astype(np.int64) for p in ref]
    bd, R0 = int(prm.bit_depth), int(prm.me_range)
    h, w = sp[0].shape
    wc, hc = (w + CTU - 1) // CTU, (h + CTU - 1) // CTU
    lam, lam_sad = int(prm.lambda_q4), int(prm.lambda_sad_q4)
    top, bottom = int(getattr(prm, "mc_top", 0)), int(getattr(prm, "mc_bottom", 0))
    cen = None if centres is None else np.asarray(centres).astype(np.int64).reshape(wc * hc, 2)
    if int(getattr(prm, "pre_search", 0)):
        cen = A.pre_search(A.lowres(sp[0], bd), A.lowres(rp[0], bd))
    cen_search = cen
    if top or bottom:
        cen_search = np.zeros((wc * hc, 2), np.int64) if cen is None else np.array(cen, np.int64)
        for i in range(len(cen_search)):
            cen_search[i, 1] = HI.clamp_centre_y(int(cen_search[i, 1]), i // wc * CTU, R0, h, top, bottom)
    table = HI.integer_table(sp[0], rp[0], bd, R0, lam_sad, cen_search, top, bottom)
    inter = HI.analyse(sp, [rp], [table], bd, int(prm.qp), int(prm.qp_c), lam_sad, lam, R0, [cen], int(getattr(prm, "rdo_zero", 0)), top, bottom,
                       rdo_cg=int(getattr(prm, "rdo_cg", 0)), sign_hide=int(getattr(prm, "sign_hide", 0)))
    # ---- what the inter program leaves per CTU
    ctus, cand = {}, np.zeros((hc, wc), bool)
    for ctu in range(wc * hc):
        x0, y0 = ctu % wc * CTU, ctu // wc * CTU
        info = inter.ctus[ctu]
        cost = tiles = act = est = 0
        for nd in info["leaves"]:
            nx, ny, n = NODES[nd]
            price, best, _ = info["rounds"][nd, 0, 1]                    # the list-0 cost the quarter round ended with
            cost += int(price[best])
            est += HI.R_CU
            for c in range(3):
                shc = 1 if c else 0
                lv = inter.coef[c][(y0 + ny) >> shc:(y0 + ny + n) >> shc, (x0 + nx) >> shc:(x0 + nx + n) >> shc]
                est += HI.R_TU + HI.sub_block_bits(lv) if lv.any() else 0
            for ty in range(0, n, 8):
                for tx in range(0, n, 8):
                    tile = sp[0][y0 + ny + ty:y0 + ny + ty + 8, x0 + nx + tx:x0 + nx + tx + 8]
                    tiles += 1
                    act += ((int(np.abs(HI.H8 @ tile @ HI.H8.T).sum()) + 2) >> 2) if activity_with_dc else hadamard_ac(tile)
        sse = 0
        for c in range(3):
            shc = 1 if c else 0
            d = (sp[c] - inter.rec[c])[y0 >> shc:(y0 + CTU) >> shc, x0 >> shc:(x0 + CTU) >> shc]
            sse += int((d * d).sum())
        t = {"cost": cost, "act": act, "tiles": tiles, "est_inter": est, "sse_inter": sse, "jinter": (sse << 4) + ((lam * est) >> 4)}
        if planted and ctu in planted:
            t.update(planted[ctu])
        first, second = t["cost"] >= (256 * t["tiles"]) << 4, t["cost"] > t["act"] << 4
        t["candidate"] = first and second
        cov["candidate", "refused by the first test" if not first else "refused by the second test" if not second else "yes"] += 1
        cov["candidate", "cost == 4 per sample"] += int(t["cost"] == (256 * t["tiles"]) << 4)
        cov["candidate", "cost == activity"] += int(t["cost"] == t["act"] << 4)
        cand[ctu // wc, ctu % wc] = t["candidate"]
        ctus[ctu] = t
    assert sum(t["est_inter"] for t in ctus.values()) == inter.est
    rounds = schedule(cand)
    # ---- the rounds
    m = IntraCodeModel(sp, prm, cov, list_from_plan)
    st = State(w, h, inter.rec, inter.cu, inter.coef)
    est, cus = inter.est, {}
    tried = [c for c in range(wc * hc) if rounds[c // wc, c % wc] >= 0]
    plans = P.IntraPlanModel(sp, bd, int(prm.tile_cols), int(prm.tile_rows)).plan(int(prm.qp), int(prm.qp_c), lam_sad, lam, int(getattr(prm, "chroma_modes", 0)), only=tried)
    for ctu in range(wc * hc):
        t = ctus[ctu]
        t["round"] = int(rounds[ctu // wc, ctu % wc])
        cov["round", {0: "0", 1: "1", -1: "never", -2: "no candidate"}[t["round"]]] += 1
    for rnd in (0, 1):
        for ctu in tried:
            t = ctus[ctu]
            if t["round"] != rnd:
                continue
            trial = st.copy()                                            # (CTUs of one round do not see each other: none is among another's four neighbours)
            info = m.code_ctu(trial, ctu, plans[ctu])
            t["j_ctu"], t["est_intra"], t["replaced"] = info["j"], info["est"], info["j"] < t["jinter"]
            cov["tried", "replaced" if t["replaced"] else "kept inter"] += 1
            cov["tried", "j_ctu == jinter"] += int(info["j"] == t["jinter"])
            cx, cy = ctu % wc, ctu // wc
            near = [ctus[(cy + dy) * wc + cx + dx] for dx, dy in ((-1, 0), (-1, -1), (0, -1), (1, -1)) if 0 <= cx + dx < wc and 0 <= cy + dy]
            if rnd == 1 and any(n.get("replaced") and n["round"] == 0 for n in near):
                cov["round-1 CTU next to a replaced round-0 CTU"] += 1
            if t["replaced"]:
                st = trial
                est += info["est"] - t["est_inter"]
                cus.update(info["cus"])
                if any(k["record"]["flags"] & F_NXN for k in info["cus"].values()):
                    cov["replaced CTU with an NxN CU"] += 1
    out = Result(st, est, cus, ctus, cov)
    out.inter, out.table, out.centres = inter, table, cen
    return out
