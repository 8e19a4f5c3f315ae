"""CPU: the encoder-side decisions that leave the stage entry points — search centres, the integer-search dump, the SAO parameters — held to
tests/hevc_analysis.py, a brute-force numpy model written from DESIGN.md §6 and not from oracle/hevc_oracle.c or the kernels.  The oracle is the
kernels' scalar twin (same SAD table, same packed ranking key, same offset walk): a rule both have wrong yields valid streams that only cost bits,
and passes every parity, syntax, reconstruction and golden test.  Here a third statement must agree with both, exactly.

First the model is pinned by answers worked out by hand.  Then model == oracle == stepped kernel sources on the cases below (shared with
tests/test_gpu_analysis_independent.py, which runs them on the device without the oracle).  Last, the rate estimate that drives rate control is
compared with what CABAC really writes."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import hevc_analysis as A
from tests import hevc_syntax as S
from tests import util
from tests.util import (ALL_SAO_KINDS, B_CASE, CODED_SAO_CASES, SAO_CASES, SEARCH_CASES, audit_search, b_case_centres, b_case_pictures, case_centres, case_pictures,
                        check_planted, first_diff, flat_pair, params_pair, periodic_pair, planes3, planted_sao_input, sao_case_sources, sao_diff, sao_kinds)


# ================================================================ hand-worked answers
def one_ctu():
    return np.zeros((32, 32), np.int64)


def test_node_order_of_the_dump():
    assert A.NODES[0] == (0, 0, 32) and A.NODES[1:5] == [(0, 0, 16), (16, 0, 16), (0, 16, 16), (16, 16, 16)]
    assert A.NODES[5:9] == [(0, 0, 8), (8, 0, 8), (0, 8, 8), (8, 8, 8)] and A.NODES[9] == (16, 0, 8) and A.NODES[20] == (24, 24, 8)
    assert [A.mvd_bits(d) for d in (0, 1, -1, 2, 3, 4, -7, 8, 128)] == [1, 3, 3, 5, 5, 7, 7, 9, 17]
    assert [A.search_span(r)[0] for r in (8, 12, 15, 32)] == [20, 28, 32, 68]


def test_one_block_with_a_known_best_match():
    """the 8x8 block at (8, 8) of the source (node 8) holds a pattern the reference holds at (13, 10): d = (+5, +2), SAD 0,
    cost = lambda (bits(20) + bits(8)) = 7 (11 + 9) = 140.  With one sample of the block 3 higher: SAD 3, cost 3 * 16 + 140 = 188."""
    rng = np.random.default_rng(1)
    pat = rng.integers(60, 250, (8, 8))
    src, ref = one_ctu(), one_ctu()
    src[8:16, 8:16] = pat
    ref[10:18, 13:21] = pat
    me = A.integer_search(src, ref, 8, 8, 7)
    assert me.shape == (1, 21, 3) and me[0, 8].tolist() == [20, 8, 140]
    assert me[0, 20].tolist() == [0, 0, 14]                       # a black block far from the pattern: the centre, 2 bits
    src[9, 9] += 3
    assert A.integer_search(src, ref, 8, 8, 7)[0, 8].tolist() == [20, 8, 188]
    # the same at 10 bit, samples x 4: the SAD is taken on the 8 high bits and scaled back: (3 << (4 + 2)) + 140
    assert A.integer_search(src * 4, ref * 4, 10, 8, 7)[0, 8].tolist() == [20, 8, 332]
    # vectors include the centre and bits are relative to it: centre (4, 1) leaves d = (1, 1): bits(4) + bits(4) = 14
    assert A.integer_search(src, ref, 8, 8, 7, [(4, 1)])[0, 8].tolist() == [20, 8, 48 + 7 * 14]
    # a picture of one 8x8 block: only the first 8x8 node exists
    me = A.integer_search(src[8:16, 8:16], ref[10:18, 13:21], 8, 8, 7)
    assert me[0, 5].tolist() == [0, 0, 48 + 14] and (me[0, np.arange(21) != 5] == (0, 0, -1)).all()


def test_flat_picture_the_centre_wins_on_bits():
    cur, ref = flat_pair(64, 64, 8)
    me = A.integer_search(cur.y, ref.y, 8, 15, 9)
    assert (me == (0, 0, 18)).all()
    me = A.integer_search(cur.y, ref.y, 8, 15, 9, np.full((4, 2), (-7, 3)))
    assert (me == (-28, 12, 18)).all()


def test_periodic_picture_the_raster_first_of_equal_costs_wins():
    cur, ref = periodic_pair(64, 64, 8)
    me = A.integer_search(cur.y, ref.y, 8, 8, 9)
    # CTU 0's nodes away from the picture's edge (reads beyond it are clamped and break the period): (-2, -2) of four equal candidates, 2 x 9 bits
    assert me[0, 8].tolist() == [-8, -8, 9 * 18] and me[0, 20].tolist() == [-8, -8, 9 * 18] and me[3, 5].tolist() == [-8, -8, 9 * 18]


def test_main10_low_bits_do_not_reach_the_sad():
    cur, ref = periodic_pair(64, 64, 10, low_bits=True)
    me = A.integer_search(cur.y, ref.y, 10, 8, 36)
    assert me[0, 8].tolist() == [-8, -8, 36 * 18] and me[3, 5].tolist() == [-8, -8, 36 * 18]


def test_low_resolution_picture_and_centres():
    y = np.zeros((8, 8), np.int64)
    y[0:4, 0:4] = np.arange(16).reshape(4, 4)                      # sum 120: (120 + 8) >> 4 = 8
    y[0:4, 4:8] = 7
    y[0, 4] = 14                                                   # sum 119: (119 + 8) >> 4 = 7
    assert A.lowres(y, 8).tolist() == [[8, 7], [0, 0]]
    y10 = np.full((4, 8), 1023, np.int64)
    y10[:, 4:] = 1021
    y10[0, 4] = 1020                                               # all 1023: (16368 + 32) >> 6 = 256, saturated; the other block: (16335 + 32) >> 6 = 255
    assert A.lowres(y10, 10).tolist() == [[255, 255]]
    assert A.lowres(np.full((4, 4), 1022), 10).tolist() == [[255]]  # a mean of 1022: (16352 + 32) >> 6 = 256: the lowest that saturates
    assert A.lowres(np.full((4, 4), 1021), 10).tolist() == [[255]] and A.lowres(np.full((4, 4), 1019), 10).tolist() == [[255]]
    assert A.lowres(np.full((4, 4), 1017), 10).tolist() == [[254]]
    # a 16x16 low-resolution picture = 2x2 CTUs; texture displaced by (+3, +2): the block of CTU 0 sits at +(3, 2) in the reference, inside it
    rng = np.random.default_rng(2)
    big = rng.integers(0, 256, (40, 40))
    lref, lsrc = big[10:26, 10:26], big[12:28, 13:29]
    assert A.pre_search(lsrc, lref)[0].tolist() == [12, 8]
    # flat: nothing to gain, the centre stays; a SAD of exactly half the zero-displacement SAD does not move it either
    assert (A.pre_search(np.full((16, 16), 9), np.full((16, 16), 40)) == 0).all()
    lsrc, lref = np.zeros((8, 16), np.int64), np.full((8, 16), 2, np.int64)
    lref[:, 8:] = 1                                                # CTU 0: SAD 128 at rest, 64 from dx = +8 on (cost 4 x 64 + 8): exactly half
    assert A.pre_search(lsrc, lref)[0].tolist() == [0, 0]
    lref[3, 12] = 0                                                # 63 at dx = +8: less than half (row 3: clamping replicates only the first and last row)
    assert A.pre_search(lsrc, lref)[0].tolist() == [32, 0]


def test_edge_categories_by_hand():
    p = np.array([[5, 5, 5, 5, 5],
                  [5, 3, 5, 7, 5],
                  [5, 5, 5, 5, 5],
                  [5, 5, 4, 4, 5]])
    k = A.edge_categories(p)
    assert (k[:, 0, :] == 0)[1:].all() and (k[:, 3, :] == 0)[1:].all()           # classes 1..3 look up or down: nothing in the first and last row
    assert (k[0, :, 0] == 0).all() and (k[0, :, 4] == 0).all()                   # class 0 looks left and right
    assert k[0, 1].tolist() == [0, 1, 0, 4, 0]                                   # 3 between 5 and 5: a minimum; 5 between 3 and 7: edgeIdx 2 + 1 - 1: none; 7: a maximum
    assert k[0, 3].tolist() == [0, 3, 2, 2, 0]                                   # 5 5 4 4 5: 5 = its left, above its right: edgeIdx 3; 4 below its left, = its right: edgeIdx 1 -> 2; 4 = left, below right: 2
    assert k[1, 1].tolist() == [0, 1, 0, 4, 0]                                   # the same minimum and maximum seen vertically
    assert k[1, 2].tolist() == [0, 3, 3, 0, 0]                                   # row 2: 5 under 3 over 5: 3; 5 under 5 over 4: 3; 5 under 7 over 4: +1 - 1: none
    assert k[2, 1].tolist() == [0, 1, 0, 4, 0]
    assert k[2, 2].tolist() == [0, 3, 4, 0, 0]                                   # 135 degrees, row 2: (5, 5, 4) -> 3; (3, 5, 4): above both -> 4; (5, 5, 5) -> 0
    assert k[3, 2].tolist() == [0, 0, 2, 3, 0]                                   # 45 degrees, a = above right, b = below left: (5, 5, 5) -> 0; (7, 5, 5) -> 2; (5, 5, 4) -> 3


def test_offset_decision_by_hand():
    # n = 10 samples that are 5 too low, lambda 40, 8 bit: o = 5 costs (250 - 500) 16 + 6 x 40 = -3760, o = 4 (160 - 400) 16 + 200 = -3640
    assert A.best_offset(10, 50, 1, 40, False, 7) == (5, -3760)
    assert A.best_offset(10, 50, -1, 40, False, 7) == (0, 40)                    # the sign rule of categories 3, 4
    assert A.best_offset(10, 50, 0, 40, True, 7) == (5, -3720)                   # a band offset also codes its sign
    assert A.best_offset(10, -50, 0, 40, True, 7) == (-5, -3720)
    assert A.best_offset(0, 0, 1, 40, False, 7) == (0, 40)
    assert A.best_offset(1, 2, 1, 16, False, 7) == (1, -16)                      # o = 1 and o = 2 both cost -16: the smaller magnitude
    assert A.best_offset(1, 100, 1, 1, False, 7) == (7, (49 - 1400) * 16 + 7)    # clipped at 7, whose truncated-unary code has 7 bins, not 8
    assert A.best_offset(1, 100, 1, 1, False, 31)[0] == 31 and A.max_offset(8) == 7 and A.max_offset(10) == 31
    # lambda decides: the mean is 2 (s / n = 20 / 10) but at lambda 700 every step costs more than it gains beyond o = 1: (10 - 40) 16 + 1400 = 920 > 700
    assert A.best_offset(10, 20, 1, 700, False, 7) == (0, 700)
    assert A.best_offset(10, 20, 1, 400, False, 7) == (1, 320)


def test_one_sao_ctu_by_hand():
    """one 32x32 picture.  Luma: flat 100 with ten isolated samples of 95 whose source is 100.  Every class sees them as category 1 (n 10, s 50 -> +5)
    and their two neighbours as category 3 with nothing to correct: every class costs 4 L + (-4000 + 6 L) + 3 L = 13 L - 4000, class 0 is first.  Band:
    band 11 (88..95) -4000 + 7 L, three more bands at L each, 7 L of signalling: 17 L - 4000, the lowest of the positions 8..11 that hold band 11.
    Cb: flat 100 against a source of 103: no edges, band 12 takes +3: (1 x 9 - 2 x 3 x 3) x 256 x 16 = -36864, + 5 L + 3 L + 7 L; Cr: flat and equal to its
    source, but it follows Cb: band, position 0 (every position costs 4 L), offsets 0."""
    L = 40
    dbk_y, src_y = np.full((32, 32), 100), np.full((32, 32), 100)
    for i in range(10):
        dbk_y[3 + 2 * (i // 5) * 7, 3 + 5 * (i % 5)] = 95
    c100, c103 = np.full((16, 16), 100), np.full((16, 16), 103)
    detail = []
    sp = A.sao_parameters((src_y, c103, c100), (dbk_y, c100, c100), 8, L, detail)
    y, cb, cr = detail[0]
    assert [k[4] for k in y] == [0, 17 * L - 4000] + [13 * L - 4000] * 4
    assert y[1][:4] == (1, 0, 8, (0, 0, 0, 5)) and y[2][:4] == (2, 0, 0, (5, 0, 0, 0))
    assert cb[1] == (1, 0, 9, (0, 0, 0, 3), -36864 + 15 * L) and [k[4] for k in cb[2:]] == [8 * L] * 4
    assert cr[1] == (1, 0, 0, (0, 0, 0, 0), 11 * L)
    o = sp[0]
    assert o["type"].tolist() == [2, 1] and o["eo_class"].tolist() == [0, 0] and o["band_pos"].tolist() == [0, 9, 0]
    assert o["offset"].tolist() == [[5, 0, 0, 0], [0, 0, 0, 3], [0, 0, 0, 0]]
    # at lambda 400 luma is not worth its bits: 13 x 400 > 4000
    assert A.sao_parameters((src_y, c103, c100), (dbk_y, c100, c100), 8, 400)[0]["type"].tolist() == [0, 1]


# ================================================================ model == oracle == stepped kernels on the cases of tests/util.py
@pytest.fixture(scope="module")
def emu():
    return util.StageApi(util.stepped_library(), "emu_")


@pytest.mark.parametrize("c", SEARCH_CASES, ids=[c.id for c in SEARCH_CASES])
def test_integer_search_model_oracle_and_stepped_kernels_agree(emu, c):
    prm, cp = params_pair(27, c.bd, c.R, pre_search=c.pre_search)
    cur, ref = case_pictures(c)
    cen = case_centres(c)
    want = audit_search(c, cur, ref, cp.lambda_sad_q4, cen)
    check_planted(c, want, cp.lambda_sad_q4)
    if c.pre_search:
        assert np.array_equal(O.search_centres(cur, ref, c.bd), A.pre_search(A.lowres(cur.y, c.bd), A.lowres(ref.y, c.bd))), "search centres: oracle != model"
    orc = O.analyze_inter(cur, ref, prm, centers=cen, dump_me=True)
    assert np.array_equal(orc.me, want), "oracle != model: " + first_diff(orc.me, want)
    got = emu.inter(cur, ref, cp, centers=cen)
    assert np.array_equal(got.me, want), "stepped kernel != model: " + first_diff(got.me, want)
    assert util.same_analysis(orc, got), util.describe_diff(orc, got)         # the rest of the analysis follows the same vectors, past the border too


def test_b_picture_both_lists(emu):
    """different displacements towards the two anchors: (+5, -3) into list 0, (-6, +4) into list 1, list 1 around explicit centres (-4, 2)"""
    c = B_CASE
    prm, cp = params_pair(27, c.bd, c.R)
    cur, ref0, ref1 = b_case_pictures()
    cen1 = b_case_centres()
    want = (A.integer_search(cur.y, ref0.y, c.bd, c.R, cp.lambda_sad_q4), A.integer_search(cur.y, ref1.y, c.bd, c.R, cp.lambda_sad_q4, cen1))
    for l, d in enumerate(c.shift):
        assert ((want[l][:, 5:, 0] == 4 * d[0]) & (want[l][:, 5:, 1] == 4 * d[1])).any(), f"list {l} misses its displacement"
    orc = O.analyze_b(cur, ref0, ref1, prm, None, cen1, dump_me=True)
    got = emu.b(cur, ref0, ref1, cp, None, cen1)
    for l in range(2):
        assert np.array_equal(orc.me[l], want[l]), f"list {l}: oracle != model: " + first_diff(orc.me[l], want[l])
        assert np.array_equal(got.me[l], want[l]), f"list {l}: stepped kernel != model: " + first_diff(got.me[l], want[l])


# ---------------------------------------------------------------- SAO
@functools.lru_cache(maxsize=None)
def oracle_sao_run(c):
    """per picture (source, deblocked, oracle parameters, model parameters); the oracle supplies the pictures, the model judges its parameters"""
    prm, cp = params_pair(c.qp, c.bd, 8)
    out, ref = [], None
    if c.content == "planted":
        src, d = planted_sao_input(c)
        return [(src, d, None, O.sao(src, d, prm)[1], A.sao_parameters(planes3(src), planes3(d), c.bd, cp.lambda_q4))]
    for i, src in enumerate(sao_case_sources(c)):
        a = O.analyze_intra(src, prm) if i == 0 else O.analyze_inter(src, ref, prm)
        d = O.deblock(a.rec, a.cu, c.bd)
        ref, sp = O.sao(src, d, prm)
        out.append((src, d, a, sp, A.sao_parameters(planes3(src), planes3(d), c.bd, cp.lambda_q4)))
    return out


@pytest.mark.parametrize("c", SAO_CASES, ids=[c.id for c in SAO_CASES])
def test_sao_parameters_model_oracle_and_stepped_kernels_agree(emu, c):
    _, cp = params_pair(c.qp, c.bd, 8)
    for i, (src, d, a, sp, want) in enumerate(oracle_sao_run(c)):
        if c.content == "rails":
            assert util.reaches_both_ends(src, c.bd, 0.01)
        assert sp.tobytes() == want.tobytes(), f"picture {i}: oracle != model: " + sao_diff(sp, want)
        got = emu.sao(src, d, cp)[1]
        assert got.tobytes() == want.tobytes(), f"picture {i}: stepped k_sao != model: " + sao_diff(got, want)
        if a is None:
            continue
        got = emu.loop_filter(src, a.rec, a.cu, cp)[1]
        assert got.tobytes() == want.tobytes(), f"picture {i}: stepped fused loop filter != model: " + sao_diff(got, want)


def test_sao_cases_reach_every_type_and_class():
    seen = set()
    for c in SAO_CASES:
        for _, _, _, sp, _ in oracle_sao_run(c):
            seen |= sao_kinds(sp)
    assert seen == ALL_SAO_KINDS, sorted(ALL_SAO_KINDS - seen)


# ================================================================ the rate estimate against what CABAC writes
def slice_data_bits(stream):
    """bits of slice_segment_data() + its trailing bits of every slice NAL unit of an Annex-B stream, by the independent reader's slice header"""
    sps, pps, out = {}, {}, []
    for nal in S.split_annexb(stream):
        t = (nal[0] >> 1) & 63
        rbsp, _ = S.nal_to_rbsp(nal[2:])
        r = S.Bits(rbsp)
        if t == 33:
            s = S.parse_sps(r)
            sps[s["id"]] = s
        elif t == 34:
            p = S.parse_pps(r)
            pps[p["id"]] = p
        elif t in (0, 1, 19, 20):
            S.slice_header(r, t, sps, pps)
            assert r.pos % 8 == 0
            out.append(8 * len(rbsp) - r.pos)
    return out


@functools.lru_cache(maxsize=None)
def estimate_run(c):
    """[(estimate in bits, real slice data bits)] for the I and the P picture of an SAO case, coded by the host coder from the oracle's analysis"""
    from hevc_amd import _lib
    lib = _lib.load()
    cfg = _lib.default_config()
    cfg.width, cfg.height, cfg.bit_depth = c.w, c.h, c.bd
    buf = (C.c_uint8 * (4 << 20))()
    n = lib.mihevc_write_parameter_sets(C.byref(cfg), buf, len(buf))
    assert n > 0
    stream, est = bytes(buf[:n]), []
    for i, (src, d, a, sp, _) in enumerate(oracle_sao_run(c)):
        n = lib.mihevc_encode_picture_host(C.byref(cfg), 2 if i == 0 else 1, i, c.qp, util.ptr(a.cu), util.ptr(a.coef_y), util.ptr(a.coef_u), util.ptr(a.coef_v),
                                           util.ptr(sp), buf, len(buf))
        assert n > 0, n
        stream += bytes(buf[:n])
        est.append(a.est / 16)
    real = slice_data_bits(stream)
    assert len(real) == len(est)
    return list(zip(est, real))


# est / real - 1 over CODED_SAO_CASES x (I, P) as measured on this path: the raw minimum and maximum.  The test below widens each by a
# quarter of itself before it compares
ESTIMATE_DEVIATION_MEASURED = (-0.3004, +0.1409)


def test_rate_estimate_against_the_coded_size():
    dev = []
    for c in CODED_SAO_CASES:
        for i, (est, real) in enumerate(estimate_run(c)):
            dev.append(est / real - 1)
            print(f"{c.id} {'IP'[i]}: estimate {est:.0f} bits, slice data {real} bits, deviation {dev[-1]:+.3f}")
    print(f"deviation min {min(dev):+.4f} max {max(dev):+.4f}")
    lo, hi = ESTIMATE_DEVIATION_MEASURED
    assert lo - abs(lo) / 4 <= min(dev) and max(dev) <= hi + abs(hi) / 4, (min(dev), max(dev))


@pytest.mark.parametrize("c", CODED_SAO_CASES, ids=[c.id for c in CODED_SAO_CASES])
def test_rate_estimate_falls_when_qp_rises_by_six(c):
    """same source and, for the P picture, the same reference: six QP steps double the quantiser step, so fewer and smaller levels survive.  Every case,
    up to QP 42 -> 48 and the rails case at 45 -> 51, the top of the range"""
    src_i, src_p = sao_case_sources(c)
    ref = oracle_sao_run(c)[0][1]
    lo, hi = params_pair(c.qp, c.bd, 8)[0], params_pair(c.qp + 6, c.bd, 8)[0]
    e = [(O.analyze_intra(src_i, p).est, O.analyze_inter(src_p, ref, p).est) for p in (lo, hi)]
    print(f"{c.id}: I {e[0][0]} -> {e[1][0]}, P {e[0][1]} -> {e[1][1]} (1/16 bit)")
    assert e[1][0] < e[0][0] and e[1][1] < e[0][1]
