"""CPU: every stream the product's host coder writes is read back by tests/hevc_syntax.py, a second reading of H.265 written independently of
hevc_amd/csrc/bitstream.cpp and oracle/hevc_dec.c, and what it reads must be exactly what the encoder decided: the CU quadtree, prediction modes,
motion, cbfs, every coefficient level, SAO, slice QP, NAL types and POCs, the entry points and the parameter sets.  The oracle decoder shares its
reading of the syntax with the writer; a shared misreading (a context offset, a candidate order, a Rice threshold) would pass every decode test
and fail here.

First the reader itself is pinned by known answers worked out by hand: Exp-Golomb codes, emulation prevention, a traced CABAC sequence, one
residual_coding, a merge list and a scaled AMVP candidate."""
import ast
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import hevc_syntax as S

HERE = Path(__file__).resolve().parent


# ================================================================ the reader is independent
# the independent modules and what each may import besides the standard library and numpy
INDEPENDENT = {"hevc_syntax.py": set(), "hevc_recon.py": {"tests.hevc_syntax", "tests.pichash_ref"}, "pichash_ref.py": set(),
               "hevc_analysis.py": {"tests.hevc_syntax", "tests.hevc_recon"},    # the numpy model of the encoder-side decisions (tests/test_analysis_independent.py)
               "sdh_ref.py": set(),                                            # the sign data hiding rule (tests/test_sign_hiding_cpu.py)
               "scene_ref.py": set(),                                          # the scene-cut sums (tests/test_gpu_scene_diff.py)
               "transform_ref.py": set(),                                      # K3 in numpy int64 (tests/test_transform_reference.py)
               "hevc_intra_plan.py": {"tests.hevc_recon", "tests.hevc_analysis", "tests.transform_ref"},    # the intra plan (tests/test_intra_plan_independent.py)
               "hevc_inter_cu.py": {"tests.hevc_recon", "tests.hevc_analysis", "tests.transform_ref", "tests.sdh_ref"},      # the inter CTU program (tests/test_inter_cu_independent.py)
               # the intra code stage, the NxN trial and the intra second pass (tests/test_intra_code_independent.py)
               "hevc_intra_code.py": {"tests.hevc_recon", "tests.hevc_analysis", "tests.transform_ref", "tests.sdh_ref", "tests.hevc_intra_plan", "tests.hevc_inter_cu"},
               "ratectl_ref.py": set()}                                        # the rate controller (tests/test_ratectl_cpu.py, tests/test_gpu_ratectl_independent.py)


def test_the_reader_imports_only_the_standard_library_and_numpy():
    """tests/hevc_syntax.py, tests/hevc_recon.py (with the stdlib-and-numpy tests/pichash_ref.py it uses), tests/hevc_analysis.py, tests/hevc_intra_plan.py and
    tests/hevc_inter_cu.py (with tests/transform_ref.py and tests/sdh_ref.py), tests/hevc_intra_code.py (on top of them), tests/scene_ref.py and tests/ratectl_ref.py load nothing of hevc_amd/ or oracle/"""
    for module, allowed in INDEPENDENT.items():
        tree = ast.parse((HERE / module).read_text())
        names = set()
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                names |= {a.name.split(".")[0] for a in node.names}
            elif isinstance(node, ast.ImportFrom):
                assert node.level == 0, "relative import in %s" % module
                if node.module == "tests":
                    names |= {"tests." + a.name for a in node.names}
                else:
                    names.add(node.module.split(".")[0])
            elif isinstance(node, ast.Call) and getattr(node.func, "id", getattr(node.func, "attr", "")) in ("__import__", "import_module", "open", "read_text"):
                pytest.fail("%s loads code or files at run time (%s)" % (module, ast.dump(node.func)))
        names.discard("__future__")
        assert names, (module, names)
        assert all(n == "numpy" or n in sys.stdlib_module_names or n in allowed for n in names), (module, names)


# ================================================================ known answers, worked by hand
def test_exp_golomb_and_fixed_length_codes():
    # 9.2: 1 -> 0, 010 -> 1, 011 -> 2, 00100 -> 3, 00111 -> 6, 0001000 -> 7; se: 1 -> 0, 010 -> 1, 011 -> -1, 00100 -> 2, 00101 -> -2
    bits = "1" "010" "011" "00100" "00111" "0001000" "1" "010" "011" "00100" "00101" "101"
    bits += "0" * (-len(bits) % 8)
    r = S.Bits(int(bits, 2).to_bytes(len(bits) // 8, "big"))
    assert [r.ue() for _ in range(6)] == [0, 1, 2, 3, 6, 7]
    assert [r.se() for _ in range(5)] == [0, 1, -1, 2, -2]
    assert r.u(3) == 5
    # 31 leading zeros: the longest ue(v) the reader accepts, 2^31 - 1 + 0
    r = S.Bits(bytes([0, 0, 0, 1, 0, 0, 0, 0]))
    assert r.ue() == (1 << 31) - 1


def test_emulation_prevention_and_rbsp_trailing_bits():
    nal = bytes([0x40, 0x01, 0x00, 0x00, 0x03, 0x01, 0x7F, 0x00, 0x00, 0x03, 0x00, 0x00, 0x03, 0x03, 0x80])
    rbsp, pos = S.nal_to_rbsp(nal)
    assert rbsp == bytes([0x40, 0x01, 0x00, 0x00, 0x01, 0x7F, 0x00, 0x00, 0x00, 0x00, 0x03, 0x80])
    assert pos == [0, 1, 2, 3, 5, 6, 7, 8, 10, 11, 13, 14, 15]          # NAL index of every RBSP byte: entry points count NAL bytes
    with pytest.raises(S.ParseError):
        S.nal_to_rbsp(bytes([0x40, 0x01, 0x00, 0x00, 0x01]))            # a start code inside a NAL unit
    r = S.Bits(bytes([0b10110000]))
    assert r.u(2) == 0b10 and r.more_rbsp_data() and r.u1() == 1 and not r.more_rbsp_data()
    r.rbsp_trailing_bits()
    stream = b"\x00\x00\x00\x01\x46\x01\x10\x00\x00\x01\x46\x01\x50\x00\x00"  # two AUDs; the zero bytes before a start code are not NAL data
    assert S.split_annexb(stream) == [b"\x46\x01\x10", b"\x46\x01\x50"]


def test_cabac_engine_trace():
    """25 bins over the bytes 90 9c 24 27 9e 98 51 d5 with one context whose initValue is 154 (part_mode, initType 1): slope 9, offset 10,
    m = 0, n = 64, preCtxState 64 -> pStateIdx 0, valMps 1 at any QP.  Traced with Tables 9-46 and 9-47 (9.3.4.3.2-9.3.4.3.5)."""
    assert S.init_context(154, 26) == [0, 1] and S.init_context(154, 51) == [0, 1]
    # merge_idx at QP 32: initType 2's 137 (m -5, n 56): preCtxState 56 - 10 = 46 -> state 17, MPS 0; initType 1's 122 (m -10, n 64): 44 -> 19, MPS 0
    assert S.init_context(137, 32) == [17, 0] and S.init_context(122, 32) == [19, 0]
    cab = S.Cabac(S.Bits(bytes.fromhex("909c24279e9851d5")), 1, 26, __import__("collections").Counter())
    assert (cab.range, cab.offset) == (510, 0b100100001)                # ivlOffset = first 9 bits = 289
    D, B, T = "D", "B", "T"
    want = [  # op, bin, pStateIdx, valMps, ivlCurrRange, ivlOffset after the bin (decisions: and after renormalisation)
        (D, 0, 0, 0, 480, 38),       # qRangeIdx 3: LPS 240, range 270 <= 289: LPS from state 0 -> valMps flips to 0; 1-bit renormalisation
        (D, 0, 1, 0, 480, 76),
        (D, 0, 2, 0, 506, 153),      # LPS 227: range 253 -> renormalised
        (D, 0, 3, 0, 290, 153),      # LPS 216: range 290, no renormalisation
        (D, 0, 4, 0, 334, 307),      # qRangeIdx 0: LPS 123, range 167
        (D, 1, 2, 0, 284, 231),      # qRangeIdx 1: LPS 142, range 192 <= 307: LPS, transIdxLps[4] = 2
        (D, 1, 1, 0, 256, 150),
        (D, 1, 0, 0, 256, 44),
        (B, 0, None, None, 256, 88),
        (B, 0, None, None, 256, 176),
        (B, 1, None, None, 256, 97),  # (176 << 1) | 1 = 353 >= 256 -> 1, offset 97
        (D, 0, 1, 0, 256, 194),
        (D, 1, 0, 0, 256, 132),
        (D, 1, 0, 1, 256, 9),        # LPS from state 0 again: valMps flips back to 1
        (D, 1, 1, 1, 256, 18),
        (D, 1, 2, 1, 256, 36),
        (D, 1, 3, 1, 256, 72),
        (D, 1, 4, 1, 266, 144),      # LPS 123 at state 3
        (D, 1, 5, 1, 300, 289),
        (B, 1, None, None, 300, 278),
        (B, 1, None, None, 300, 256),
        (D, 0, 4, 1, 444, 271),      # LPS 111 at state 5: range 111 -> 222 -> 444, a 2-bit renormalisation
        (D, 1, 5, 1, 275, 271),      # qRangeIdx 2: LPS 169, range 275, no renormalisation
        (T, 0, None, None, 273, 271),  # terminate: range 273 > 271 -> 0, no renormalisation needed
        (T, 1, None, None, 271, 271),  # range 271 <= 271 -> 1 (end of the arithmetic code)
    ]
    for k, (op, b, st, mps, rng, off) in enumerate(want):
        got = cab.decision("part_mode", 0) if op == D else cab.bypass() if op == B else cab.terminate()
        state = tuple(cab.ctx["part_mode"][0])
        assert (got, cab.range, cab.offset) == (b, rng, off), (k, op, got, cab.range, cab.offset)
        if op == D:
            assert state == (st, mps), (k, state)
    assert cab.r.pos == 31 and len(want) >= 20


class ScriptedBins:
    """stands in for the arithmetic decoder: hands out bins from a script and records which (syntax element, ctxInc) asked for each"""

    def __init__(self, bins):
        self.bins, self.log = list(bins), []

    def decision(self, name, inc):
        self.log.append((name, inc))
        return self.bins.pop(0)

    def bypass(self):
        self.log.append("bypass")
        return self.bins.pop(0)

    def bypass_bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bypass()
        return v


def test_residual_coding_4x4_with_an_escape_and_a_rising_rice_parameter():
    """inter luma 4x4 (diagonal scan) with levels 40 at (2,0), 3 at (0,1), 1 at (1,0), -7 at (0,2), -1 at (0,0): scan positions 5, 1, 2, 3, 0.
    last x prefix 2 = TR '110' (ctxInc 0,1,2: ctxOffset 0, ctxShift 0), last y prefix 0 = '0'; sig_coeff_flag n = 4..0 at ctxIdxMap 3, 6, 1, 2, 0;
    greater1: ctxSet 0, greater1Ctx 1, 0, 0, 0, 0; greater2 on scan position 5; signs; then coeff_abs_level_remaining:
      n5: baseLevel 3, rem 37 with cRiceParam 0: prefix '1111' (cMax 4) + EG1 of 33: '1111' '0' '00011' -> 8 ones, an escape
      n3: baseLevel 2, rem 5 with cRiceParam 1 (40 > 3 * 2^0): TR '110' + '1'
      n1: baseLevel 2, rem 1 with cRiceParam 2 (7 > 3 * 2^1): '0' + '01'"""
    bins = [1, 1, 0, 0]                      # last_sig_coeff_x_prefix, last_sig_coeff_y_prefix
    bins += [0, 1, 1, 1, 1]                  # sig_coeff_flag n = 4, 3, 2, 1, 0
    bins += [1, 1, 0, 1, 0]                  # coeff_abs_level_greater1_flag n = 5, 3, 2, 1, 0
    bins += [1]                              # coeff_abs_level_greater2_flag n = 5
    bins += [0, 1, 0, 0, 1]                  # coeff_sign_flag n = 5, 3, 2, 1, 0
    bins += [1, 1, 1, 1] + [1, 1, 1, 1, 0] + [0, 0, 0, 1, 1]     # n5 remaining: 37
    bins += [1, 1, 0, 1]                     # n3 remaining: 5
    bins += [0, 0, 1]                        # n1 remaining: 1
    cab = ScriptedBins(bins)
    dec = S.SliceDecoder.__new__(S.SliceDecoder)
    dec.cab = cab
    out = dec.residual_block(2, 0, None)
    assert not cab.bins
    want = np.zeros((4, 4), np.int32)
    want[0, 2], want[1, 0], want[0, 1], want[2, 0], want[0, 0] = 40, 3, 1, -7, -1
    assert np.array_equal(out, want), out
    ctx = [e for e in cab.log if e != "bypass"]
    assert ctx == [("last_sig_coeff_x_prefix", 0), ("last_sig_coeff_x_prefix", 1), ("last_sig_coeff_x_prefix", 2), ("last_sig_coeff_y_prefix", 0),
                   ("sig_coeff_flag", 3), ("sig_coeff_flag", 6), ("sig_coeff_flag", 1), ("sig_coeff_flag", 2), ("sig_coeff_flag", 0),
                   ("coeff_abs_level_greater1_flag", 1), ("coeff_abs_level_greater1_flag", 0), ("coeff_abs_level_greater1_flag", 0),
                   ("coeff_abs_level_greater1_flag", 0), ("coeff_abs_level_greater1_flag", 0), ("coeff_abs_level_greater2_flag", 0)]
    # the same bins as chroma: sig_coeff_flag + 27, greater1 + 16, greater2 + 4, last prefix ctxOffset 15
    cab = ScriptedBins(bins)
    dec.cab = cab
    assert np.array_equal(dec.residual_block(2, 1, None), want)
    ctx = [e for e in cab.log if e != "bypass"]
    assert ctx[:4] == [("last_sig_coeff_x_prefix", 15), ("last_sig_coeff_x_prefix", 16), ("last_sig_coeff_x_prefix", 17), ("last_sig_coeff_y_prefix", 15)]
    assert [i for _, i in ctx[4:9]] == [30, 33, 28, 29, 27] and [i for _, i in ctx[9:14]] == [17, 16, 16, 16, 16] and ctx[14][1] == 4


def test_residual_coding_4x4_with_a_hidden_sign():
    """sign data hiding on, inter luma 4x4 (diagonal scan) with levels at scan positions 9, 4 and 0: (x 3, y 0) = 2, (1, 1) = -1 and (0, 0) = ?.
    lastSigScanPos 9 - firstSigScanPos 0 = 9 > 3: signHidden, so coeff_sign_flag is coded for n = 9 and 4 only and the sign at n = 0 is inferred
    from sumAbsLevel (7.4.9.11).  last x prefix 3 = '111' (cMax 3), last y prefix 0 = '0'; sig_coeff_flag n = 8..0; greater1 on n = 9, 4, 0 (flags 1, 0,
    0), greater2 on n = 9 (0): |levels| 2, 1, 1, no coeff_abs_level_remaining.  sumAbsLevel 4 is even: the level at n = 0 stays +1.  With a third
    level of 1 at n = 0 replaced by a remaining escape of 1 (|level| 2 there, sum 5, odd) it becomes -2."""
    lead = [1, 1, 1, 0]                                             # last_sig_coeff_x_prefix '111', last_sig_coeff_y_prefix '0'
    sig = [0, 0, 0, 0, 1, 0, 0, 0, 1]                               # sig_coeff_flag n = 8 .. 0
    for g1_0, rem, want0 in ((0, [], 1), (1, [0], -2)):
        bins = lead + sig + [1, 0, g1_0] + [0] + [0, 1]              # greater1 n = 9, 4, 0; greater2 n = 9; signs n = 9 (+), 4 (-)
        bins += rem                                                  # n = 0 with greater1: baseLevel 2 = 1 + 1 + 0 (not first greater1): TR '0' -> 0
        cab = ScriptedBins(bins)
        dec = S.SliceDecoder.__new__(S.SliceDecoder)
        dec.cab, dec.sign_hiding = cab, 1
        out = dec.residual_block(2, 0, None)
        assert not cab.bins, cab.bins
        want = np.zeros((4, 4), np.int32)
        want[0, 3], want[1, 1], want[0, 0] = 2, -1, want0
        assert np.array_equal(out, want), out
    # the same bins without sign data hiding leave one bin unread (the coded sign of n = 0) and then run out
    dec = S.SliceDecoder.__new__(S.SliceDecoder)
    dec.cab = ScriptedBins(lead + sig + [1, 0, 0] + [0] + [0, 1] + [1])
    out = dec.residual_block(2, 0, None)
    assert out[0, 0] == -1 and not dec.cab.bins


def neighbourhood(poc, ref_pocs, motions, slice_type=0, max_merge=5):
    """a 64x64 picture of four CTBs, one slice, one tile; the current PU is the 16x16 block at (32, 32) of CTB 3, so that all five spatial
    neighbours (in CTBs 0, 1 and 2) precede it.  motions: {(x, y): Mot or None (intra)} for 4x4 blocks"""
    sps = {"width": 64, "height": 64, "ctb_log2": 5, "bit_depth_luma": 8}
    pps = {"tile_cols": 1, "tile_rows": 1, "uniform_spacing_flag": 1, "log2_parallel_merge_level": 2}
    lay = S.Layout(sps, pps)
    pic = S.Picture(sps, pps, 0, poc)
    pic.ctb_slice = [0, 0, 0, 0]
    hdr = {"slice_type": slice_type, "max_num_merge_cand": max_merge, "num_ref_idx": (1, 1 if slice_type == 0 else 0), "slice_addr_rs": 0}
    dec = S.SliceDecoder(pic, sps, pps, lay, hdr, b"", [], 0, ref_pocs, None)
    for (x, y), m in motions.items():
        i = (y >> 2) * lay.w4 + (x >> 2)
        pic.st_mode[i], pic.st_mot[i] = ("inter", m) if m is not None else ("intra", None)
    return dec


def test_merge_list_of_a_hand_drawn_b_neighbourhood():
    """B slice, POC 2 between RefPicList0[0] = POC 0 and RefPicList1[0] = POC 4; MaxNumMergeCand 5.
      A1 (31, 47): L0 (4, -2)           -> candidate 0
      B1 (47, 31): L0 (4, -2)           -> same motion as A1: pruned
      B0 (48, 31): L0 (4, -2)           -> compared with B1 (available, though pruned): same motion, pruned
      A0 (31, 48): L1 (-6, 8)           -> differs from A1: candidate 1
      B2 (31, 31): L0 (4, -2)           -> same as A1: pruned
    combined (Table 8-6): combIdx 0 = (l0Cand 0, l1Cand 1): L0 (4, -2) + L1 (-6, 8), the two lists name different pictures -> candidate 2;
    combIdx 1 = (1, 0): candidate 1 has no L0 -> none; numOrigMergeCand * (numOrigMergeCand - 1) = 2 reached.
    zero candidates: bi-predictive, refIdx 0 in both lists (numRefIdx = 1) -> candidates 3 and 4."""
    M = S.Mot
    l0 = M((1, 0), ((4, -2), (0, 0)), (0, -1))
    dec = neighbourhood(2, (0, 4), {(31, 47): l0, (47, 31): l0, (48, 31): l0, (31, 48): M((0, 1), ((0, 0), (-6, 8)), (-1, 0)), (31, 31): l0})
    got = dec.merge_list(32, 32, 16, 32, 32, 16, 16, 0)
    want = [l0, M((0, 1), ((0, 0), (-6, 8)), (-1, 0)), M((1, 1), ((4, -2), (-6, 8)), (0, 0)), M((1, 1), ((0, 0), (0, 0)), (0, 0)),
            M((1, 1), ((0, 0), (0, 0)), (0, 0))]
    assert got == want, got
    # B2 only joins when fewer than four of A0, A1, B0, B1 made it; in a P slice zero candidates are L0-only and there is no combined one
    dec = neighbourhood(3, (2, None), {(31, 47): l0, (47, 31): M((1, 0), ((1, 1), (0, 0)), (0, -1)), (48, 31): None, (31, 48): None,
                                       (31, 31): M((1, 0), ((-3, 0), (0, 0)), (0, -1))}, slice_type=1, max_merge=4)
    got = dec.merge_list(32, 32, 16, 32, 32, 16, 16, 0)
    assert got == [l0, M((1, 0), ((1, 1), (0, 0)), (0, -1)), M((1, 0), ((-3, 0), (0, 0)), (0, -1)), M((1, 0), ((0, 0), (0, 0)), (0, -1))], got


def test_amvp_candidates_scaled_between_different_poc_distances():
    """B slice at POC 5, RefPicList0[0] = POC 4, RefPicList1[0] = POC 8; AMVP for list 0 (target POC 4, tb = 1).
    A1 uses only list 1 (POC 8), so no A neighbour names POC 4: A1's vector is scaled (8.5.3.2.7, 8.5.3.2.8) with td = 5 - 8 = -3:
      tx = (16384 + 1) / -3 = -5461, distScaleFactor = (1 * -5461 + 32) >> 6 = -85,
      mv = (-85 * -37 = 3145 -> (3145 + 127) >> 8 = 12, -85 * 21 = -1785 -> -((1785 + 127) >> 8) = -7) = (12, -7).
    B1 uses list 0 (POC 4): (3, 3) unscaled.  isScaledFlag is 1 (A1 available), so B is not scaled again."""
    M = S.Mot
    assert S.scale_mv((-37, 21), -3, 1) == (12, -7)
    dec = neighbourhood(5, (4, 8), {(31, 47): M((0, 1), ((0, 0), (-37, 21)), (-1, 0)), (47, 31): M((1, 0), ((3, 3), (0, 0)), (0, -1))})
    assert dec.amvp_list(32, 32, 16, 32, 32, 16, 16, 0, 0) == [(12, -7), (3, 3)]
    # no A neighbour at all: B1's vector is copied to A (8-185); B is then derived again with scaling (td = tb = 1: factor 256, the same vector),
    # equals A and is dropped; a zero vector fills the list
    dec = neighbourhood(5, (4, 8), {(47, 31): M((1, 0), ((3, 3), (0, 0)), (0, -1))})
    assert dec.amvp_list(32, 32, 16, 32, 32, 16, 16, 0, 0) == [(3, 3), (0, 0)]
    # the distance clip: td = -200 clips to -128, tb = 100 stays; tx = (16384 + 64) / -128 = -128, factor = (100 * -128 + 32) >> 6 = -200
    assert S.scale_mv((64, -1), -200, 100) == (-50, 1)
    assert (S.wrap16(32767 + 1), S.wrap16(-32768 - 1), S.wrap16(100)) == (-32768, 32767, 100)


# ================================================================ the host coder's streams against the encoder's decisions
def expect_cell(rec, slice_type):
    """the fields of one parsed 8x8 record that the analysis record determines"""
    fl = int(rec["flags"])
    inter = fl & 1
    want = {"log2": int(rec["log2_size"]), "inter": inter, "cbf_y": (fl >> 1) & 1, "cbf_cb": (fl >> 2) & 1, "cbf_cr": (fl >> 3) & 1}
    if not inter:
        want.update(nxn=(fl >> 4) & 1, cmode=int(rec["chroma_mode"]), imode=[int(m) for m in rec["intra_mode"]])
        if fl & 16:
            want["cbf_y4"] = int(rec["cbf_y4"])
    else:
        l1 = slice_type == 0 and (fl & 32) != 0
        l0 = not (slice_type == 0 and (fl & 64))
        want.update(pf0=int(l0), pf1=int(l1))
        if l0:
            want.update(mv0x=int(rec["mvx"]), mv0y=int(rec["mvy"]))
        if l1:
            m = rec["intra_mode"]
            s16 = lambda lo, hi: ((int(lo) | (int(hi) << 8)) ^ 0x8000) - 0x8000        # little-endian int16 in the intra_mode bytes
            want.update(mv1x=s16(m[0], m[1]), mv1y=s16(m[2], m[3]))
    return want


def check_picture(pic, a, sao, qp, slice_type, nal_type, poc, rows=None):
    """one parsed picture (or the CTU rows `rows` of it, for a slice) against the analysis, SAO parameters and QP it was coded from"""
    y0, y1 = (0, pic.h) if rows is None else rows
    assert pic.nal_type == nal_type and pic.poc == poc, (pic.nal_type, pic.poc, nal_type, poc)
    sl = [s for s in pic.slices if y0 <= (s["address"] // ((pic.w + 31) >> 5)) * 32 < y1]
    assert sl and all(s["slice_type"] == slice_type and s["slice_qp"] == qp for s in sl), [(s["slice_type"], s["slice_qp"]) for s in sl]
    assert (a.cu["qp"] == qp).all()                              # cu_qp_delta is off: QpY = SliceQpY everywhere
    g = pic.cu
    h8, w8 = a.cu.shape
    for by in range(h8):
        for bx in range(w8):
            want = expect_cell(a.cu[by, bx], slice_type)
            gy = by + (y0 >> 3)
            got = {k: (list(g[k][gy, bx]) if k == "imode" else int(g[k][gy, bx])) for k in want}
            assert got == want, "picture POC %d, 8x8 block (%d, %d): parsed %s, analysis %s" % (poc, bx * 8, by * 8, got, want)
            n = 1 << int(a.cu[by, bx]["log2_size"])
            x, y = bx * 8, gy * 8
            if int(a.cu[by, bx]["flags"]) & 1 and x % n == 0 and (by * 8) % n == 0:
                # the encoder's policy checked against the independently derived merge list: merge with the first candidate that carries the CU's
                # motion, skip when that holds and the CU has no residual
                mine = S.Mot((want["pf0"], want["pf1"]), ((want.get("mv0x", 0), want.get("mv0y", 0)), (want.get("mv1x", 0), want.get("mv1y", 0))),
                             (0 if want["pf0"] else -1, 0 if want["pf1"] else -1))
                lst = pic.merge_lists[(x, y)]
                idx = next((i for i, m in enumerate(lst) if m == mine), -1)
                resid = want["cbf_y"] or want["cbf_cb"] or want["cbf_cr"]
                assert (int(g["merge_flag"][gy, bx]), int(g["merge_idx"][gy, bx]), int(g["skip"][gy, bx])) == \
                       (int(idx >= 0), idx, int(idx >= 0 and not resid)), (poc, x, y, lst, mine)
    ch0, ch1 = y0 >> 1, y1 >> 1
    assert np.array_equal(pic.coef[0][y0:y1], a.coef_y), "luma levels differ (POC %d)" % poc
    assert np.array_equal(pic.coef[1][ch0:ch1], a.coef_u) and np.array_equal(pic.coef[2][ch0:ch1], a.coef_v), "chroma levels differ (POC %d)" % poc
    wc = (pic.w + 31) >> 5
    ctbs = range((y0 >> 5) * wc, ((y1 + 31) >> 5) * wc)
    if sao is None:
        assert all(not s["header"]["slice_sao_luma_flag"] and not s["header"]["slice_sao_chroma_flag"] for s in sl)
    else:
        for k, rs in enumerate(ctbs):
            got, want = pic.sao[rs], sao[k]
            for c in range(3):
                t = int(want["type"][min(c, 1)])
                assert got["type"][min(c, 1)] == t, (poc, rs, c, got, want)
                if t:
                    assert got["offset"][c] == [int(v) for v in want["offset"][c]], (poc, rs, c, got, want)
                if t == 1:
                    assert got["band_pos"][c] == int(want["band_pos"][c]), (poc, rs, c, got, want)
                if t == 2:
                    assert got["eo_class"][min(c, 1)] == int(want["eo_class"][min(c, 1)]), (poc, rs, c, got, want)


def check_stream(st, coded):
    """coded: per picture in decoding order (analysis, SAO parameters or None, QP, slice type, NAL type, POC)"""
    assert len(st.pictures) == len(coded)
    for pic, (a, sao, qp, stype, nal, poc) in zip(st.pictures, coded):
        check_picture(pic, a, sao, qp, stype, nal, poc)


def dpb_needs(st):
    """(largest number of pictures the decoder must hold: the RPS plus the current picture, reorder depth in output order)"""
    dpb = max(len(p.rps_all) + 1 for p in st.pictures)
    reorder, pocs = 0, []
    for i, p in enumerate(st.pictures):          # pictures before it in decoding order that follow it in output order (within its CVS)
        cvs = [q for q in st.pictures[:i] if q.poc > p.poc and not any(r.nal_type in (19, 20) for r in st.pictures[st.pictures.index(q) + 1:i + 1])]
        reorder = max(reorder, len(cvs))
    return dpb, reorder


def check_parameter_sets(st, cfg, grids):
    from hevc_amd import _lib
    sps = st.sps[0]
    cw, chh = (cfg.width + 7) & ~7, ((cfg.pic_height or cfg.height) + 7) & ~7
    assert (sps["width"], sps["height"]) == (cw, chh)
    assert sps["conf_win"] == (0, (cw - cfg.width) // 2, 0, (chh - (cfg.pic_height or cfg.height)) // 2)
    assert sps["bit_depth_luma"] == cfg.bit_depth and sps["ptl"]["profile_idc"] == (2 if cfg.bit_depth == 10 else 1)
    assert sps["ptl"]["compat"] == (0x20000000 if cfg.bit_depth == 10 else 0x60000000)
    assert sps["ptl"]["level_idc"] == cfg.level_idc and sps["ptl"]["tier_flag"] == cfg.tier
    assert all(v["ptl"]["level_idc"] == cfg.level_idc for v in st.vps.values())
    vui = sps["vui"]
    assert (vui["colour_primaries"], vui["transfer_characteristics"], vui["matrix_coeffs"], vui["video_full_range_flag"]) == \
           (cfg.colour_primaries, cfg.transfer, cfg.matrix, cfg.full_range)
    assert (vui["num_units_in_tick"], vui["time_scale"]) == (cfg.fps_den, cfg.fps_num)
    if cfg.hrd:
        hrd = vui["hrd"]
        e = hrd["sub_layers"][0]["nal"][0]
        assert (e["bit_rate_value_minus1"] + 1) << (6 + hrd["bit_rate_scale"]) == cfg.vbv_maxrate_kbps * 1000
        assert (e["cpb_size_value_minus1"] + 1) << (4 + hrd["cpb_size_scale"]) == cfg.vbv_bufsize_kbits * 1000
    else:
        assert vui["hrd"] is None
    assert 1 << sps["log2_max_poc_lsb"] > 2 * max(p.poc for p in st.pictures)
    used = {(p.slices[0]["pps_id"], p.slices[0]["slice_type"] == 2) for p in st.pictures}
    for pps_id, idr in used:
        pps = st.pps[pps_id]
        assert (pps["tile_cols"], pps["tile_rows"]) == (grids[0] if idr else grids[1]), (pps_id, idr)
        assert pps["uniform_spacing_flag"] == 1
    dpb, reorder = dpb_needs(st)
    o = sps["ordering"][-1]
    assert o["max_dec_pic_buffering_minus1"] + 1 >= dpb and o["max_num_reorder_pics"] >= reorder, (o, dpb, reorder)
    assert len(st.aud) == (len(st.pictures) if cfg.aud else 0)


def pictures_case(name, w, h, qp, bd, n, keyint, content="synth", nxn=0, intra_in_p=0, **kw):
    from hevc_amd import _lib
    from tests import util
    from tests.test_bitstream_cpu import encode_pictures, flashing_clip, make_cfg, occluded_clip
    cfg = make_cfg(w, h, bd, **kw)
    if content == "synth":
        srcs = [util.synth_frame(h, w, seed=11, shift=(3 * i, i), bit_depth=bd) for i in range(n)]
    elif content == "full_range":
        srcs = flashing_clip(w, h, bd, n)
    elif content == "occluded":
        srcs = occluded_clip(w, h, bd, n)
    elif content == "still":
        still = util.synth_frame(h, w, seed=2, detail=False)
        srcs = [still.copy() for _ in range(n)]
    else:
        hh = (h + 7) & ~7
        ww = (w + 7) & ~7
        srcs = [util.synth_frame(hh, ww, seed=6, shift=(2 * i, i), bit_depth=bd) for i in range(n)]
    _, stream, recs, packets = encode_pictures(cfg, srcs, qp, bd, keyint=keyint, nxn=nxn, intra_in_p=intra_in_p)
    coded = []
    for i, (a, sao, q) in enumerate(zip(encode_pictures.last_analyses, encode_pictures.last_saos, encode_pictures.last_qps)):
        intra = i % keyint == 0
        coded.append((a, sao, q, 2 if intra else 1, 19 if intra else 1, i % keyint))
    return cfg, stream, coded, (_lib.tile_grid(cfg), _lib.p_tile_grid(cfg)), recs


def b_case(name, w, h, qp, bd, n, aud, content="synth"):
    from hevc_amd import _lib
    from tests import util
    from tests.test_bitstream_cpu import encode_gop_with_b, flashing_clip, make_cfg
    cfg = make_cfg(w, h, bd, aud=aud, bframes=1)
    if content == "synth":
        srcs = [util.synth_frame(h, w, seed=17, shift=(3 * i, 2 * i), bit_depth=bd) for i in range(n)]
    else:
        srcs = flashing_clip(w, h, bd, n)
    stream, recs, types, _ = encode_gop_with_b(cfg, srcs, qp, bd)
    coded = [(a, sao, q, st, {2: 19, 1: 1, 0: 0}[st], pos) for pos, st, a, sao, q in encode_gop_with_b.last_coded]
    return cfg, stream, coded, (_lib.tile_grid(cfg), _lib.p_tile_grid(cfg)), [recs[pos] for pos, _, _, _, _ in encode_gop_with_b.last_coded]


def sliced_case(name, w, h, bd, rows, level, keyint, n=3):
    """test_sliced_cpu's pipeline: every band of CTU rows is coded by its own session as a slice of the whole picture"""
    from hevc_amd import _lib
    from oracle import oracle as O
    from tests import util
    from tests.test_sliced_cpu import band_frames, sliced_cfg
    lib = _lib.load()
    _, bands = band_frames(h, w, rows, n, bd)
    buf = (C.c_uint8 * (4 << 20))()
    cfgs = [sliced_cfg(w, h, bd, rows, k, level, aud=1) for k in range(len(rows))]
    m = lib.mihevc_write_parameter_sets(C.byref(cfgs[0]), buf, len(buf))
    heads = bytes(buf[:m])
    prm_i, prm_p = O.default_params(24, bd, 12), O.default_params(27, bd, 12)
    refs, stream, coded, recs = [None] * len(rows), b"", [], []
    for i in range(n):
        intra = i % keyint == 0
        per = []
        for k, cfg in enumerate(cfgs):
            prm = O.Params.from_buffer_copy(bytes(prm_i if intra else prm_p))
            prm.mc_top, prm.mc_bottom = int(k > 0), int(k < len(rows) - 1)
            if intra:
                prm.tile_cols, prm.tile_rows = _lib.tile_grid(cfg)
            a = O.analyze_intra(bands[k][i], prm) if intra else O.analyze_inter(bands[k][i], refs[k], prm)
            refs[k], sao = O.sao(bands[k][i], O.deblock(a.rec, a.cu, bd), prm)
            m = lib.mihevc_encode_picture_host(C.byref(cfg), 2 if intra else 1, i % keyint, prm.qp, util.ptr(a.cu), util.ptr(a.coef_y),
                                               util.ptr(a.coef_u), util.ptr(a.coef_v), util.ptr(sao), buf, len(buf))
            assert m > 0
            pkt = bytes(buf[:m])
            if k == 0:
                cut = pkt.index(b"\0\0\0\1", 4)
                pkt = pkt[:cut] + (heads if i == 0 else b"") + pkt[cut:]
            else:
                pkt = pkt[pkt.index(b"\0\0\0\1", 4):]
            stream += pkt
            per.append((a, sao, prm.qp))
        coded.append((per, 2 if intra else 1, 19 if intra else 1, i % keyint))
        recs.append(O.Frame(*(np.vstack([getattr(r, c) for r in refs]) for c in "yuv")))
    full = sliced_cfg(w, h, bd, rows, 0, level, aud=1)
    return full, stream, coded, (_lib.tile_grid(cfgs[0]), _lib.p_tile_grid(cfgs[0])), recs


def hash_case(name, w, h, qp, bd, n, pic_hash, **kw):
    """pictures_case with a decoded picture hash SEI (hash_type pic_hash - 1, written by the product's SEI writer) behind every picture, of the
    oracle pipeline's reconstruction.  No AUDs: the repository's decoder reads a suffix SEI behind the slices only without them (as in
    tests/test_gpu_pichash.py)"""
    from hevc_amd import _lib
    from tests import pichash_ref as R
    from tests import util
    from tests.test_bitstream_cpu import encode_pictures, make_cfg
    cfg = make_cfg(w, h, bd, aud=0, pic_hash=pic_hash, **kw)
    srcs = [util.synth_frame(h, w, seed=13, shift=(3 * i, 2 * i), bit_depth=bd) for i in range(n)]
    headers, _, recs, packets = encode_pictures(cfg, srcs, qp, bd, keyint=1000, nxn=1, intra_in_p=1)
    lib, buf = _lib.load(), (C.c_uint8 * 256)()
    stream, coded = b"", []
    for i, ((pkt, _, intra), a, sao, q) in enumerate(zip(packets, encode_pictures.last_analyses, encode_pictures.last_saos, encode_pictures.last_qps)):
        if i == 0:
            pkt = headers + pkt
        vals = R.picture_hash([recs[i].y, recs[i].u, recs[i].v], bd, pic_hash - 1)
        raw = (C.c_uint8 * 48)(*b"".join(vals)) if pic_hash == 1 else (C.c_uint32 * 3)(*vals)
        m = lib.mihevc_write_picture_hash_sei(C.byref(cfg), pic_hash - 1, raw, buf, len(buf))
        assert m > 0, m
        stream += pkt + bytes(buf[:m])
        coded.append((a, sao, q, 2 if intra else 1, 19 if intra else 1, i))
    return cfg, stream, coded, (_lib.tile_grid(cfg), _lib.p_tile_grid(cfg)), recs


def sdh_case(name, w, h, qp, bd, n=3, content="synth"):
    """test_sign_hiding_cpu's pictures: the kernel sources stepped on the CPU with sign_hide = 1 (I, P with NxN, the intra second pass and
    rdo_cg, then a B picture), coded by the product's host coder"""
    from hevc_amd import _lib
    from oracle import oracle as O
    from tests import util
    from tests.test_sign_hiding_cpu import S as SDH
    cfg = _lib.default_config()
    cfg.width, cfg.height, cfg.bit_depth, cfg.me_range, cfg.qp, cfg.keyint, cfg.bframes = w, h, bd, 8, qp, 5, 1
    cfg.intra_nxn, cfg.intra_in_p, cfg.rdo_cg, cfg.pre_search, cfg.sign_hide, cfg.level_idc = 1, 1, 5, 0, 1, 93
    srcs = [util.content_frame(content, h, w, seed=3, shift=(2 * i, i), bit_depth=bd) for i in range(n)]
    pics = SDH.stepped_pictures(util.StageApi(util.stepped_library(), "emu_", sign_hide=1), cfg, srcs, [0], qp)
    buf = (C.c_uint8 * (1 << 16))()
    m = _lib.load().mihevc_write_parameter_sets(C.byref(cfg), buf, len(buf))
    stream, coded, recs = bytes(buf[:m]), [], []
    for i, st, pkt, a, rec in pics:
        q = max(0, qp - 3) if st == 2 else qp + 2 if st == 0 else qp
        _, sao = O.sao(srcs[i], O.deblock(a.rec, a.cu, bd), SDH.params(cfg, q, st == 2))
        stream += pkt
        coded.append((a, sao, q, st, {2: 19, 1: 1, 0: 0}[st], i))
        recs.append(rec)
    return cfg, stream, coded, (_lib.tile_grid(cfg), _lib.p_tile_grid(cfg)), recs


def drawn_intra_case(name, w, h, qp, bd):
    """CU records drawn by hand and given straight to the host coder: two IDR pictures of 32x32 and then 16x16 intra CUs whose luma modes run
    through 0..34 in raster order (chroma in DM, so its 16x16 and 8x8 TBs see every mode too), random low-frequency levels in every TB, and SAO
    band offset in every CTB with sao_band_position 29, 30 and 31, where the four bands wrap round to 0.  The encoder's own search does not reach
    every mode at every size.  No oracle pipeline made these pictures: the reconstruction to compare with is the repository decoder's."""
    from hevc_amd import _lib
    from oracle import oracle as O
    from tests import util
    from tests.test_bitstream_cpu import make_cfg
    cfg = make_cfg(w, h, bd, aud=1)
    lib = _lib.load()
    buf = (C.c_uint8 * (4 << 20))()
    m = lib.mihevc_write_parameter_sets(C.byref(cfg), buf, len(buf))
    headers = bytes(buf[:m])
    rng = np.random.default_rng(7)
    cmax = (1 << (min(bd, 10) - 5)) - 1
    stream, coded = b"", []
    for i, log2 in enumerate((5, 4)):
        a = O.Analysis(h, w)
        n = 1 << log2
        for k, (y0, x0) in enumerate((y, x) for y in range(0, h, n) for x in range(0, w, n)):
            mode = k % 35
            flags = 0
            for c, (plane, tb) in enumerate(((a.coef_y, n), (a.coef_u, n // 2), (a.coef_v, n // 2))):
                yc, xc = (y0, x0) if c == 0 else (y0 // 2, x0 // 2)
                lv = rng.integers(-4, 5, (4, 4)) * (rng.random((4, 4)) < 0.5)
                plane[yc:yc + 4, xc:xc + 4] = lv
                flags |= int(lv.any()) << (c + 1)
            r = a.cu[y0 // 8:(y0 + n) // 8, x0 // 8:(x0 + n) // 8]
            r["log2_size"], r["flags"], r["qp"], r["intra_mode"], r["chroma_mode"] = log2, flags, qp, mode, mode
        nctb = ((w + 31) // 32) * ((h + 31) // 32)
        sao = np.zeros(nctb, O.SAO_DTYPE)
        for rs in range(nctb):
            sao[rs]["type"] = (1, 1)
            sao[rs]["band_pos"] = (29 + rs % 3, 29 + (rs + 1) % 3, 29 + (rs + 2) % 3)
            sao[rs]["offset"] = rng.integers(-cmax, cmax + 1, (3, 4))
        m = lib.mihevc_encode_picture_host(C.byref(cfg), 2, 0, qp, util.ptr(a.cu), util.ptr(a.coef_y), util.ptr(a.coef_u), util.ptr(a.coef_v),
                                           util.ptr(sao), buf, len(buf))
        assert m > 0, m
        pkt = bytes(buf[:m])
        if i == 0:
            cut = pkt.index(b"\0\0\0\1", 4)
            pkt = pkt[:cut] + headers + pkt[cut:]
        stream += pkt
        coded.append((a, sao, qp, 2, 19, 0))
    return cfg, stream, coded, (_lib.tile_grid(cfg), _lib.p_tile_grid(cfg)), None


from tests.test_bitstream_cpu import ENVELOPE_STREAM_CASES, STREAM_CASES  # noqa: E402

CASES = {}
for c in STREAM_CASES:
    CASES["stream-" + "-".join(map(str, c))] = (pictures_case, dict(w=c[0], h=c[1], qp=c[2], bd=c[3], n=c[4], keyint=c[5], aud=1))
for c in ENVELOPE_STREAM_CASES:
    CASES["envelope-" + "-".join(map(str, c))] = (pictures_case, dict(w=c[0], h=c[1], qp=c[2], bd=c[3], n=c[4], keyint=c[5], content="full_range", aud=1))
CASES.update({
    "idr-tiles-512x64": (pictures_case, dict(w=512, h=64, qp=30, bd=8, n=3, keyint=2, level_idc=120)),
    "idr-tiles-256x128-10bit": (pictures_case, dict(w=256, h=128, qp=28, bd=10, n=2, keyint=2, level_idc=150)),
    "p-tiles-512x64": (pictures_case, dict(w=512, h=64, qp=30, bd=8, n=3, keyint=3, level_idc=120, p_tiles=1, aud=1)),
    "p-tiles-intra-256x128": (pictures_case, dict(w=256, h=128, qp=34, bd=8, n=3, keyint=3, level_idc=150, p_tiles=1, intra_in_p=1, content="occluded")),
    "nxn-64x64": (pictures_case, dict(w=64, h=64, qp=22, bd=8, n=2, keyint=1, nxn=1)),
    "nxn-136x72": (pictures_case, dict(w=136, h=72, qp=30, bd=8, n=2, keyint=1, nxn=1)),
    "nxn-72x104-10bit": (pictures_case, dict(w=72, h=104, qp=18, bd=10, n=2, keyint=1, nxn=1)),
    "intra-in-p-136x104": (pictures_case, dict(w=136, h=104, qp=24, bd=8, n=3, keyint=1000, nxn=1, intra_in_p=1, content="occluded")),
    "intra-in-p-128x96-10bit": (pictures_case, dict(w=128, h=96, qp=30, bd=10, n=3, keyint=1000, intra_in_p=1, content="occluded")),
    "sao-off-still": (pictures_case, dict(w=96, h=64, qp=32, bd=8, n=3, keyint=1000, sao=0, content="still")),
    "off-grid-100x60": (pictures_case, dict(w=100, h=60, qp=30, bd=8, n=2, keyint=1000, content="offgrid")),
    "hdr10-64x64": (pictures_case, dict(w=64, h=64, qp=24, bd=10, n=2, keyint=1000, hdr10=1, colour_primaries=9, transfer=16, matrix=9, chroma_loc=0,
                                        aud=1, repeat_headers=1, level_idc=150, hrd=1, vbv_maxrate_kbps=11760, vbv_bufsize_kbits=14112)),
    "b-96x80": (b_case, dict(w=96, h=80, qp=26, bd=8, n=7, aud=1)),
    "b-136x72-noaud": (b_case, dict(w=136, h=72, qp=32, bd=8, n=6, aud=0)),
    "b-72x104-10bit": (b_case, dict(w=72, h=104, qp=24, bd=10, n=5, aud=1)),
    "b-160x96-qp20": (b_case, dict(w=160, h=96, qp=20, bd=8, n=5, aud=1)),
    "b-96x80-qp0-full_range": (b_case, dict(w=96, h=80, qp=0, bd=8, n=5, aud=1, content="full_range")),
    "sliced-160x96": (sliced_case, dict(w=160, h=96, bd=8, rows=(2, 1), level=63, keyint=3)),
    "sliced-96x160-10bit": (sliced_case, dict(w=96, h=160, bd=10, rows=(1, 2, 2), level=63, keyint=2)),
    "sdh-64x64": (sdh_case, dict(w=64, h=64, qp=30, bd=8)),
    "sdh-72x104-10bit": (sdh_case, dict(w=72, h=104, qp=26, bd=10)),
    "drawn-intra-224x160": (drawn_intra_case, dict(w=224, h=160, qp=30, bd=8)),
    "hash-md5-96x80": (hash_case, dict(w=96, h=80, qp=27, bd=8, n=3, pic_hash=1)),
    "hash-crc-72x104-10bit": (hash_case, dict(w=72, h=104, qp=25, bd=10, n=3, pic_hash=2)),
    "hash-checksum-136x72": (hash_case, dict(w=136, h=72, qp=32, bd=8, n=3, pic_hash=3)),
})


@functools.lru_cache(maxsize=None)
def encoded(name):
    """(configuration, stream, per picture what was coded, tile grids, the oracle pipeline's reconstructions in decoding order)"""
    fn, kw = CASES[name]
    return fn(name, **kw)


@functools.lru_cache(maxsize=None)
def parsed(name):
    cfg, stream, coded, grids, _ = encoded(name)
    return cfg, S.parse_stream(stream), coded, grids


@pytest.mark.parametrize("name", sorted(CASES))
def test_parsed_stream_equals_the_encoder_decisions(name):
    cfg, st, coded, grids = parsed(name)
    if CASES[name][0] is sliced_case:
        rows = CASES[name][1]["rows"]
        assert len(st.pictures) == len(coded)
        wc = (cfg.width + 31) >> 5
        for pic, (per, stype, nal, poc) in zip(st.pictures, coded):
            assert [s["address"] for s in pic.slices] == [sum(rows[:k]) * wc for k in range(len(rows))]
            y0 = 0
            for k, (a, sao, qp) in enumerate(per):
                y1 = y0 + a.coef_y.shape[0]
                check_picture(pic, a, sao, qp, stype, nal, poc, rows=(y0, y1))
                y0 = y1
            # each band is filtered as a picture of its own: in-loop filters never cross a slice edge
            assert all(s["header"]["slice_loop_filter_across_slices_enabled_flag"] == 0 for s in pic.slices[1:])
    else:
        check_stream(st, coded)
    check_parameter_sets(st, cfg, grids)
    if name.startswith("b-"):
        kinds = set()
        for pic in st.pictures:
            if pic.slices[0]["slice_type"] == 0:
                inter = pic.cu["inter"] == 1
                kinds |= set(zip(pic.cu["pf0"][inter].tolist(), pic.cu["pf1"][inter].tolist()))
        assert kinds == {(1, 0), (0, 1), (1, 1)}, kinds
    if "tiles" in name:
        assert any(len(s["header"]["entry_point_offsets"]) > 0 for p in st.pictures for s in p.slices)
    if name.startswith("hdr10"):
        sei = {m["type"]: m for _, msgs in st.sei for m in msgs}
        assert sei[137]["primaries"] == [(13250, 34500), (7500, 3000), (34000, 16000)] and sei[137]["white_point"] == (15635, 16450)
        assert (sei[137]["max_luminance"], sei[137]["min_luminance"]) == (10000000, 50)
        assert (sei[144]["max_content_light_level"], sei[144]["max_pic_average_light_level"]) == (1000, 400)
        assert st.sps[0]["vui"]["chroma_sample_loc_type_top_field"] == 0
    if name == "sao-off-still":
        assert all(p.cu["skip"].all() for p in st.pictures[1:])
    pps_flags = {st.pps[s["pps_id"]]["sign_data_hiding_enabled_flag"] for p in st.pictures for s in p.slices}
    assert pps_flags == {int(name.startswith("sdh-"))}
    if name.startswith("hash-"):
        kind = CASES[name][1]["pic_hash"] - 1
        assert all(p.hash is not None and p.hash[0] == kind for p in st.pictures)
        assert all(m["type"] == 132 for t, msgs in st.sei if t == 40 for m in msgs)
    else:
        assert all(p.hash is None for p in st.pictures)


# Contexts the emitted subset can never reach, with the reason.  Every other (syntax element, ctxInc, initType) of the reader's tables must be decoded
# at least once over the cases above: a wrong initValue anywhere else would change a decoded bin somewhere.
UNREACHABLE = {
    ("split_transform_flag", None, None): "max_transform_hierarchy_depth_inter/intra are 0: the flag is never signalled (NxN splits by inference)",
    ("part_mode", (1, 2, 3), None): "bins after the first belong to non-2Nx2N inter partitions and AMP, never coded",
    ("cbf_chroma", (1, 2, 3), None): "chroma cbfs at trafoDepth > 0 need a transform split of a CU of 16 or more",
    ("inter_pred_idc", (3,), None): "CtDepth 3 needs an 8x8 CU in a 64x64 CTB; CTBs are 32",
    ("inter_pred_idc", None, 1): "initType 1 holds B slices only with cabac_init_flag = 1, and the PPS never allows cabac_init_flag",
    ("sig_coeff_flag", tuple(range(15, 21)), 2): "mode-dependent 8x8 luma scans are intra-only, and B pictures carry no intra CU",
    ("sig_coeff_flag", tuple(range(1, 9)), 2): "luma 4x4 TBs come only from intra NxN, and B pictures carry no intra CU",
    ("last_sig_coeff_x_prefix", (0, 1, 2), 2): "luma 4x4 TBs come only from intra NxN, and B pictures carry no intra CU",
    ("last_sig_coeff_y_prefix", (0, 1, 2), 2): "luma 4x4 TBs come only from intra NxN, and B pictures carry no intra CU",
    ("cbf_luma", (0,), 2): "cbf_luma at trafoDepth 1 comes only from intra NxN, and B pictures carry no intra CU",
    ("prev_intra_luma_pred_flag", None, 2): "B pictures carry no intra CU",
    ("intra_chroma_pred_mode", None, 2): "B pictures carry no intra CU",
}


def unreachable(name, inc, it):
    for (n, incs, its), _ in UNREACHABLE.items():
        if n == name and (incs is None or inc in incs) and (its is None or it == its):
            return True
    return False


def test_every_reachable_context_is_decoded():
    hits = __import__("collections").Counter()
    for name in CASES:
        hits.update(parsed(name)[1].hits)
    missing = []
    for name, per_type in S.CTX_INIT.items():
        for it, vals in enumerate(per_type):
            if vals is None:
                continue
            for inc in range(len(vals)):
                if not unreachable(name, inc, it) and hits[(name, inc, it)] == 0:
                    missing.append((name, inc, it))
    assert not missing, missing
    assert not [k for k in hits if unreachable(*k)], "a context listed as unreachable was decoded"


def test_hand_drawn_b_picture_reaches_a_combined_candidate_and_a_large_scaled_predictor():
    """CU records drawn by hand and given straight to the host coder (I0, P2, then B1 between them; 64x64, 16x16 CUs, no residual, SAO off).
    The encoder's own B decisions rarely land on a combined bi-predictive candidate, and with the two pictures one POC away on either side
    the AMVP scaling factor is -256, so a wrong rounding only shows on vectors of 128 quarter samples or more.  Here:
      CU (16, 16): A1 = CU (0, 16) bi L0 (4, 0) / L1 (-4, 0), B1 = CU (16, 0) bi L0 (8, 8) / L1 (-8, -8), B0 = CU (32, 0) = B1 and
        B2 = CU (0, 0) = A1 are pruned; combined: combIdx 0 -> L0 (4, 0) + L1 (-8, -8), combIdx 1 -> L0 (8, 8) + L1 (-4, 0).  The CU carries
        L0 (8, 8) / L1 (-4, 0) and no residual: skip with merge_idx 3.
      CU (48, 16): L0 (-200, 160); its A1, CU (32, 16), uses list 1 only with (200, -160) -> the first AMVP candidate is that vector scaled from
        POC distance -1 to +1: (-200, 160), an exact predictor."""
    from hevc_amd import _lib
    from oracle import oracle as O
    from tests import util
    from tests.test_bitstream_cpu import make_cfg
    lib = _lib.load()
    w = h = 64
    cfg = make_cfg(w, h, 8, bframes=1, sao=0)
    buf = (C.c_uint8 * (1 << 20))()
    n = lib.mihevc_write_parameter_sets(C.byref(cfg), buf, len(buf))
    stream = bytes(buf[:n])
    qp = 30

    def record(kind):
        a = O.Analysis(h, w)
        a.cu["qp"] = qp
        if kind == "I":
            a.cu["log2_size"], a.cu["intra_mode"], a.cu["chroma_mode"] = 5, 1, 1
        else:
            a.cu["log2_size"], a.cu["flags"] = 4, 1
        return a

    def inter(a, cx, cy, l0=None, l1=None):
        r = a.cu[2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2]
        r["flags"] = 1 | (32 if l1 else 0) | (0 if l0 else 64)
        r["mvx"], r["mvy"] = l0 if l0 else (0, 0)
        if l1:
            v = [(l1[0] & 255), (l1[0] >> 8) & 255, (l1[1] & 255), (l1[1] >> 8) & 255]
            r["intra_mode"] = v

    b = record("B")
    inter(b, 0, 0, (4, 0), (-4, 0))
    inter(b, 1, 0, (8, 8), (-8, -8))
    inter(b, 2, 0, (8, 8), (-8, -8))
    inter(b, 0, 1, (4, 0), (-4, 0))
    inter(b, 1, 1, (8, 8), (-4, 0))
    inter(b, 2, 1, None, (200, -160))
    inter(b, 3, 1, (-200, 160), None)
    coded = []
    for st, pos, a in ((2, 0, record("I")), (1, 2, record("P")), (0, 1, b)):
        m = lib.mihevc_encode_picture_host(C.byref(cfg), st, pos, qp, util.ptr(a.cu), util.ptr(a.coef_y), util.ptr(a.coef_u), util.ptr(a.coef_v), None,
                                           buf, len(buf))
        assert m > 0, m
        stream += bytes(buf[:m])
        coded.append((a, None, qp, st, {2: 19, 1: 1, 0: 0}[st], pos))
    s = S.parse_stream(stream)
    check_stream(s, coded)
    g = s.pictures[2].cu
    assert (int(g["skip"][2, 2]), int(g["merge_idx"][2, 2])) == (1, 3)
    assert (int(g["merge_flag"][2, 6]), int(g["mvp0"][2, 6]), int(g["mv0x"][2, 6]), int(g["mv0y"][2, 6])) == (0, 0, -200, 160)
