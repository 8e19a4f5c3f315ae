"""CPU: everything the inter CTU program (`inter_ctu_program`: `k_inter_ctu`, `k_inter_ctu_b`) decides after the integer search — quadtree, half- and
quarter-sample vectors, the list choice of B pictures, the RD zero-out, records, levels, reconstruction, rate estimate — held to tests/hevc_inter_cu.py,
a brute-force numpy model written from DESIGN.md §6 ("Decision rules of the inter CTU program, in words") and not from oracle/hevc_oracle.c or the kernel.
The oracle is the kernel's scalar twin (same ring table, same packed key, same bottom-up pass): a rule both have wrong yields a valid stream that decodes to
the encoder's own reconstruction and only costs bits or quality.

First hand-worked pictures, each through the model, the oracle and the stepped kernel in three lane orders (the last of them: the coefficient-group drop of
`rdo_cg` at, below and above the exact equality of its comparison).  Then model == oracle == stepped kernel on util.INTER_CASES, every case in full (shared with
tests/test_gpu_inter_cu_independent.py, which runs them on the device without the oracle), sign data hiding behind the group drop (model == stepped kernel), what
the MODEL reached over them — on the residual-rich cases: groups dropped and kept at every plane and TU size, TUs emptied, ties of both zero-outs — and the footprint
property of motion-constrained slices."""
import collections

import numpy as np
import pytest

from oracle import oracle as O
from tests import hevc_analysis as A
from tests import hevc_inter_cu as M
from tests import util
from tests.test_sliced_cpu import mv_rows_ok
from tests.util import GROUP_PINS, INTER_CASES, INTER_COVERAGE, INTER_PINS, PIN_B_MVS, PIN_MVS, PIN_SPLIT_MVS, RICH_CASES, SATD_ROUNDING_CASES, SIGN_HIDE_CASES, inter_case_params, inter_case_want, inter_diff, run_inter_case

LANE_ORDERS = (("0", None), ("1", None), ("2", "11"))          # sequential, reversed, random lane order (the last over random initial LDS)


@pytest.fixture(scope="module")
def emu():
    return util.StageApi(util.stepped_library(), "emu_")


def held(emu, monkeypatch, name):
    """the model's analysis of a hand-made case, after the oracle AND the stepped kernel source (in the three lane orders) have been held to it"""
    c = INTER_PINS[name]
    want = inter_case_want(c)[0]
    d = inter_diff(want, run_inter_case(O, c))
    assert not d, "oracle != model: " + d
    for order, fill in LANE_ORDERS:
        monkeypatch.setenv("EMU_ORDER", order)
        if fill:
            monkeypatch.setenv("EMU_SHARED_FILL", fill)
        d = inter_diff(want, run_inter_case(emu, c))
        assert not d, f"stepped kernel (lane order {order}) != model: " + d
    monkeypatch.delenv("EMU_SHARED_FILL", raising=False)
    return want, inter_case_params(c)[1].lambda_sad_q4


def bits(mv):
    return A.mvd_bits(mv[0]) + A.mvd_bits(mv[1])


# ================================================================ hand-worked answers
def hadamard_sum_by_hand(d):
    """sum |H d H^T| of an 8x8 block by the definition, entry by entry: H[i][j] = (-1)^popcount(i & j); not normalised"""
    h = [[-1 if bin(i & j).count("1") & 1 else 1 for j in range(8)] for i in range(8)]
    return sum(abs(sum(h[u][y] * int(d[y][x]) * h[v][x] for y in range(8) for x in range(8))) for u in range(8) for v in range(8))


def test_the_parts_by_hand():
    d = np.zeros((8, 8), np.int64)
    d[0, 0] = 3                                              # one sample: all 64 coefficients are +-3: (192 + 2) >> 2
    assert M.satd(d) == 48
    assert M.satd(np.full((8, 8), 1)) == 16                  # a constant: the DC coefficient alone, 64: (64 + 2) >> 2
    d[0, 1], d[1, 0] = 3, 6                                  # 3 (1 + h[v][1] + 2 h[u][1]): 12 on 16 coefficients, 6 on 16, 0 on 16, 6 on 16 = 384 -> 96
    assert M.satd(d) == 96
    # normalised PER TILE: a 16x16 block is the sum of its four tiles' rounded values, not the rounded sum
    big = np.random.default_rng(0).integers(-40, 41, (16, 16))         # tile sums 9612, 9750, 9956, 10782: 10026 per tile, 10025 at once
    raw = [hadamard_sum_by_hand(big[y:y + 8, x:x + 8]) for y in (0, 8) for x in (0, 8)]
    assert M.satd(big) == sum((r + 2) >> 2 for r in raw) != (sum(raw) + 2) >> 2
    # footprints: 8 rows at row 0; a whole-sample vector reads its own rows, a fraction 3 above and 4 below; chroma (eighth samples) 1 above and 2 below
    assert M.rows_inside(0, 8, 0, 64, 1, 1) and not M.rows_inside(0, 8, 2, 64, 1, 1) and M.rows_inside(0, 8, 2, 64, 0, 1)
    assert M.rows_inside(3, 8, 2, 64, 1, 0) and not M.rows_inside(2, 8, 2, 64, 1, 0)          # rows 3 - 3 = 0 .. : inside; 2 - 3: outside
    assert M.rows_inside(4, 8, 4, 64, 1, 0) is True                                          # one whole sample down: luma rows 5..12; chroma vector 4/8: a fraction: rows 2 - 1 .. : inside
    assert not M.rows_inside(0, 8, 4, 64, 1, 0)                                              # the same at row 0: luma is whole-sample, but CHROMA has the fraction 4/8 and reads row -1
    assert M.rows_inside(56, 8, 0, 64, 0, 1) and not M.rows_inside(56, 8, 1, 64, 0, 1) and M.rows_inside(48, 8, 18, 64, 0, 1) and not M.rows_inside(48, 8, 21, 64, 0, 1)
    assert M.clamp_centre_y(-20, 32, 8, 96, 1, 0) == -20 and M.clamp_centre_y(-40, 32, 8, 96, 1, 0) == -24 and M.clamp_centre_y(30, 32, 8, 96, 0, 1) == 24
    assert M.clamp_centre_y(5, 64, 8, 72, 0, 1) == -8                                        # the last CTU row of a 72-row picture has 8 rows: 72 - 72 - 8
    # levels 1 and 2 in two sub-blocks, -6 in a third: 53 + 27 floor(log2 5) = 107
    assert M.sub_block_bits(np.array([[1, 0, 0, 0, 2, 0, 0, 0]] + [[0] * 8] * 3 + [[0, 0, 0, 0, -6, 0, 0, 0]] + [[0] * 8] * 3)) == 143 + 33 + 143 + 50 + 143 + 107


def test_a_flat_pair_the_centre_wins_both_rounds_and_the_ctu_stays_whole(emu, monkeypatch):
    """every prediction equals the source: SATD 0 everywhere, so every cost is its bits.  Node cost 2 L; a 16x16 stays whole at 6 L against 2 L + 4 x 6 L,
    the 32x32 at 6 L against 2 L + 4 x 6 L = 26 L; every ring candidate costs bits(+-2) or bits(+-1) more than the centre; no residual: 80 per CU."""
    want, lam = held(emu, monkeypatch, "pin-flat")
    for t in want.ctus:
        assert t["leaves"] == [0] and t["mv"][0] == [(0, 0)] and t["tree"][-1] == (6 * lam, 26 * lam) and t["tree"][0] == (6 * lam, 26 * lam)
        for rnd in (0, 1):
            price, best, _ = t["rounds"][0, 0, rnd]
            step = 2 - rnd
            assert best == 0 and price == [2 * lam] + [lam * bits((dx * step, dy * step)) for dx, dy in M.RING]
    assert want.est == 4 * 80 and (want.cu["flags"] == 1).all() and (want.cu["log2_size"] == 5).all() and not any(c.any() for c in want.coef)


@pytest.mark.parametrize("name", ["pin-planted", "pin-main10"])
def test_planted_half_and_quarter_sample_vectors_are_found_at_satd_zero(emu, monkeypatch, name):
    """every 32x32 block of the source IS the reference at one vector through 8.5.3.3.3: (13, -9) and (7, -3) (quarter samples in both directions), (14, -8)
    (a half sample in x), (-2, 6) (half samples in both).  Wherever the integer search lands, the two rings must arrive there, where the SATD is 0 and the
    cost is the vector's bits; the two quarter-sample CTUs stay whole, from (12, -8) and (8, -4): the centre wins the half round, ring positions 3 and 6 the
    quarter round."""
    want, lam = held(emu, monkeypatch, name)
    planted = PIN_MVS[::2]
    for t, mv in zip(want.ctus, planted):
        for nd in t["leaves"]:
            assert t["mv"][nd] == [mv] and t["rounds"][nd, 0, 1][0][t["rounds"][nd, 0, 1][1]] == lam * bits(mv), (nd, t["mv"][nd])
    assert want.ctus[0]["leaves"] == [0] and [want.ctus[0]["rounds"][0, 0, r][1] for r in (0, 1)] == [0, 3]
    assert want.ctus[3]["leaves"] == [0] and [want.ctus[3]["rounds"][0, 0, r][1] for r in (0, 1)] == [0, 6]
    assert want.ctus[1]["leaves"] == [0] and want.ctus[1]["rounds"][0, 0, 0][1] in (4, 5) and want.ctus[1]["rounds"][0, 0, 1][1] == 0      # (12 or 16, -8) -> (14, -8), then it stays
    assert (want.cu["flags"] == 1).all() and not any(c.any() for c in want.coef)


def test_four_quadrants_that_move_differently_split_the_ctu(emu, monkeypatch):
    want, lam = held(emu, monkeypatch, "pin-split")
    for i, t in enumerate(want.ctus):
        assert t["leaves"] == [1, 2, 3, 4] and t["tree"][-1][0] > t["tree"][-1][1]
        for q in range(4):
            blk = (2 * (i // 2) + q // 2) * 4 + 2 * (i % 2) + q % 2                       # the 16x16 block's raster number in the 64x64 picture
            mv = PIN_SPLIT_MVS[2 * blk % len(PIN_SPLIT_MVS)]
            assert t["mv"][1 + q] == [mv] and t["rounds"][1 + q, 0, 1][0][t["rounds"][1 + q, 0, 1][1]] == lam * bits(mv)
    assert want.est == 16 * 80 and (want.cu["log2_size"] == 4).all()


def test_b_picture_the_average_of_two_anchors_takes_both_lists(emu, monkeypatch):
    """the source is the default weighted average of anchor 0 at (5, 2) and anchor 1 at (-3, 6); the anchors differ by noise, so each list alone keeps an
    error and the average has none: key = L (bits0 + bits1) + L"""
    want, lam = held(emu, monkeypatch, "pin-b-both")
    assert all(m == M.BI for t in want.ctus for m in t["mode"].values())
    for i in (1, 3):                                                                          # the CTUs away from the left edge, which the list-1 vector reads across
        t = want.ctus[i]
        assert t["leaves"] == [0] and t["mv"][0] == [PIN_B_MVS[0], PIN_B_MVS[1]] and t["keys"][0][2] == lam * (12 + 12) + lam == min(t["keys"][0])
    assert (want.cu["flags"] & 0x60 == 0x20).all() and (want.cu["mvx"][:, 4:] == 5).all()
    assert (want.cu["intra_mode"][:, 4:] == (253, 255, 6, 0)).all()                  # the list-1 vector, two little-endian int16


@pytest.mark.parametrize("name,mode", [("pin-b-list0", M.L0), ("pin-b-list1", M.L1)])
def test_b_picture_one_list_alone_wins_where_the_source_is_that_anchor(emu, monkeypatch, name, mode):
    want, lam = held(emu, monkeypatch, name)
    mv = PIN_B_MVS[mode]
    for t in want.ctus:
        for nd in t["leaves"]:
            assert t["mode"][nd] == mode and t["mv"][nd][mode] == mv and t["keys"][nd][mode] == lam * bits(mv) + 2 * lam == min(t["keys"][nd])
    r = want.cu
    if mode == M.L0:                  # the unused list reports a zero vector
        assert (r["flags"] == 1).all() and (r["intra_mode"] == 0).all() and (r["mvx"] == mv[0]).all() and (r["mvy"] == mv[1]).all()
    else:
        assert (r["flags"] == 0x61).all() and (r["mvx"] == 0).all() and (r["mvy"] == 0).all() and (r["intra_mode"] == (mv[0] & 255, 255, mv[1], 0)).all()


# ================================================================ the coefficient-group drop (rdo_cg), by hand
def planted_groups(want, c):
    """(the model's group table of the TU the case's residual was planted in, that block's CU records)"""
    _, x, y, n, _, _ = c.plant[0]
    ctu = y // 32 * 2 + x // 32
    nd = [k for k, (nx, ny, nn) in enumerate(M.NODES) if (nx, ny, nn) == (x % 32, y % 32, n)][0]
    assert nd in want.ctus[ctu]["leaves"], "the planted block is not a CU of its own"
    assert set(want.ctus[ctu]["groups"]) == {(nd, 0)} and all(not t["groups"] for i, t in enumerate(want.ctus) if i != ctu), "a level outside the planted luma TU"
    return want.ctus[ctu]["groups"][nd, 0], want.cu[y >> 3:(y + n) >> 3, x >> 3:(x + n) >> 3]


@pytest.mark.parametrize("name", list(GROUP_PINS))
def test_a_group_is_kept_at_equality_and_dropped_one_step_of_lambda_later(emu, monkeypatch, name):
    """every block of the picture is the reference at its own vector, so the only residual is the constant planted on one block: one coefficient, (0, 0), one level,
    one group.  rdo_cg = 2: the group's lambda is lambda_q4 (lambda_q4 x 2 >> 1).  bits = 33 (a level of 1) + 143 = 176, so ((lambda x 176) >> 4) = 11 lambda exactly.

    8x8, 8 bit, QP 32, residual 4: rows 64 x 8 x 4 = 2048, (+ 2) >> 2 = 512; columns 64 x 8 x 512, (+ 256) >> 9: c = 512.  Quantiser: 32 % 6 = 2: 20560, qbits = 14 + 5 + 4 = 23,
      (512 x 20560 + (85 << 14)) >> 23 = 11919360 >> 23 = 1.  Scaled: ((16 x 51 << 5) + 32) >> 6 = 26144 >> 6: r = 408.  D = 408 x (1024 - 408) = 251328, 16 D = 4021248.
      Threshold: 11 lambda << 2 (15 - 8 - 3) = 2816 lambda: 4021248 at lambda_q4 = 1428.
    8x8, 10 bit, QP 24, residual 8: rows 4096, >> 4: 256; columns 64 x 8 x 256 >> 9: c = 256.  qP = 36: 26214, qbits = 14 + 6 + 2 = 22, (256 x 26214 + (85 << 13)) >> 22 = 7407104 >> 22 = 1.
      Scaled: ((16 x 40 << 6) + 128) >> 8: r = 160.  D = 160 x (512 - 160) = 56320, 16 D = 901120.  Threshold: 11 lambda << 4 = 176 lambda: 901120 at 5120.
    32x32, 8 bit, QP 32, residual 1: rows 64 x 32 = 2048, >> 4: 128; columns 64 x 32 x 128 >> 11: c = 128.  qbits = 14 + 5 + 2 = 21, (128 x 20560 + (85 << 12)) >> 21 = 2979840 >> 21 = 1.
      Scaled: (26112 + 128) >> 8: r = 102.  D = 102 x (256 - 102) = 15708, 16 D = 251328.  Threshold: 11 lambda << 4 (the shift is 2 (15 - 8 - 5) = 4): 251328 at 1428.
    32x32, 10 bit, QP 24, residual 2: rows 4096, >> 6: 64; columns 64 x 32 x 64 >> 11: c = 64.  qbits = 14 + 6 + 0 = 20, (64 x 26214 + (85 << 11)) >> 20 = 1851776 >> 20 = 1.
      Scaled: (40960 + 512) >> 10: r = 40.  D = 40 x (128 - 40) = 3520, 16 D = 56320.  Threshold: 11 lambda, NOT shifted (2 (15 - 10 - 5) = 0): 56320 at 5120.
    At equality and one below the group stays (`<`), one above it goes: the TU's only group, so its cbf is 0, the record says so and the estimate loses R_TU + 176."""
    bd, _, _, plant, qp, lq = GROUP_PINS[name]
    D, shift = {"8x8-8bit": (251328, 8), "8x8-10bit": (56320, 4), "32x32-8bit": (15708, 4), "32x32-10bit": (3520, 0)}[name]
    est = {}
    for tag, lam_q4 in (("below", lq - 1), ("equal", lq), ("above", lq + 1)):
        c = INTER_PINS[f"pin-cg-{name}-{tag}"]
        want, _ = held(emu, monkeypatch, c.id)
        groups, rec = planted_groups(want, c)
        assert groups == {(0, 0): (D, 176, (11 * lam_q4) << shift, tag == "above")}
        assert (16 * D == (11 * lam_q4) << shift) == (tag == "equal")
        assert (rec["flags"] == (M.F_INTER if tag == "above" else M.F_INTER | M.F_CBF[0])).all()
        assert (want.cu["flags"] & 0xe != 0).sum() == (0 if tag == "above" else rec.size) and not want.coef[1].any() and not want.coef[2].any()
        assert int(np.count_nonzero(want.coef[0])) == (0 if tag == "above" else 1)
        est[tag] = want.est
    assert est["below"] == est["equal"] == est["above"] + M.R_TU + 176
    _, x, y, n, dc, _ = c.plant[0]                                                                # dropped: the block reconstructs to its prediction, the picture without the plant
    assert np.array_equal(want.rec[0][y:y + n, x:x + n], np.asarray(util.inter_case_pictures(c)[0].y, np.int64)[y:y + n, x:x + n] - dc)


def test_of_two_groups_one_is_dropped_and_the_cbf_stays(emu, monkeypatch):
    """8x8, 8 bit, QP 32, lambda_q4 = 1500, residual 4 + 8 x (+ - - + + - - +) by rows: every row is constant, 12 or -4: rows 64 x 8 x 12 >> 2 = 1536 and -512 in column 0;
    columns: v = 0: 64 x (4 x 1536 - 4 x 512) = 262144, >> 9: 512; v = 4 (64 x the same signs): 64 x (4 x 1536 + 4 x 512) = 524288, >> 9: 1024; the other rows are
    orthogonal to both.  Group (0, 0) is the one of the test above: 16 D = 4021248 < 2816 x 1500 = 4224000: dropped.  Group (1, 0): (1024 x 20560 + (85 << 14)) >> 23 =
    22446080 >> 23 = 2; r = (2 x 26112 + 32) >> 6 = 816; D = 816 x (2048 - 816) = 1005312, 16 D = 16084992; bits = 50 + 143 = 193, threshold ((1500 x 193) >> 4) << 8 =
    18093 << 8 = 4631808: kept.  The TU keeps its cbf and costs 30 + 193."""
    c = INTER_PINS["pin-cg-one-of-two"]
    want, _ = held(emu, monkeypatch, c.id)
    groups, rec = planted_groups(want, c)
    assert groups == {(0, 0): (251328, 176, 4224000, True), (1, 0): (1005312, 193, 4631808, False)}
    assert (rec["flags"] == M.F_INTER | M.F_CBF[0]).all() and int(np.count_nonzero(want.coef[0])) == 1 and want.coef[0][20, 16] == 2
    assert want.est == inter_case_want(INTER_PINS["pin-cg-8x8-8bit-above"])[0].est + M.R_TU + 193


# ================================================================ model == oracle == stepped kernel
@pytest.mark.parametrize("c", INTER_CASES, ids=[c.id for c in INTER_CASES])
def test_model_oracle_and_stepped_kernel_agree(emu, c):
    want, me, _ = inter_case_want(c)
    orc, got = run_inter_case(O, c), run_inter_case(emu, c)
    for l, m in enumerate(me):
        for name, a in (("oracle", orc), ("stepped kernel", got)):
            t = a.me if len(me) == 1 else a.me[l]
            assert np.array_equal(t, m), f"integer table, list {l}: {name} != model: " + util.first_diff(t, m)
    d = inter_diff(want, orc)
    assert not d, "oracle != model: " + d
    d = inter_diff(want, got)
    assert not d, "stepped kernel != model: " + d


def test_sign_hiding_behind_the_group_drop_model_and_stepped_kernel_agree():
    """the oracle has no sign data hiding and the device's frame stage entries take no switch for it, so this is the model against the stepped kernels alone:
    the parity rule (tests/sdh_ref.py) after the group decisions and before the TU zero-out, on four residual-rich pictures"""
    api = util.StageApi(util.stepped_library(), "emu_", sign_hide=1)
    cov = collections.Counter()
    assert {(c.bd, c.content.startswith("b-"), c.rdo_cg) for c in SIGN_HIDE_CASES} == {(8, True, 5), (8, True, 0), (10, False, 5), (10, False, 0)}
    for c in SIGN_HIDE_CASES:
        want = inter_case_want(c, 1)[0]
        d = inter_diff(want, run_inter_case(api, c))
        assert not d, f"{c.id}: stepped kernel with sign hiding != model: " + d
        assert inter_diff(want, run_inter_case(O, c)), "sign hiding changed nothing"
        cov.update(INTER_COVERAGE[c.id + "+sdh"])
    assert cov["sign hiding adjusted a group"] >= 50 and cov["sign hiding adjusted a group", "in a TU that lost a group"] >= 1, cov


def test_the_cases_are_the_ones_asked_for():
    plain = {(c.w, c.h, c.bd, c.R, c.qp, c.rdo_zero) for c in INTER_CASES if c.content.startswith("warp") and c.lam is None and c.mc == (0, 0) and not c.rdo_cg}
    assert plain >= {(w, h, bd, R, qp, rz) for (w, h) in util.SIZES for bd in (8, 10) for R in (8, 15) for qp in (22, 32, 42) for rz in (0, 1)}
    assert {c.mc for c in INTER_CASES} == {(0, 0), (1, 0), (0, 1), (1, 1)} and any(c.pre_search for c in INTER_CASES) and any(c.centres == "corners" for c in INTER_CASES)
    assert any(c.lam and c.lam[0] == 0 for c in INTER_CASES) and any(c.content.startswith("b-") for c in INTER_CASES)
    # the residual-rich pictures: the three sizes x both depths, QP 22 and 27, the three grids and a B picture, rdo_cg 2 / 5 / 8 with the TU zero-out on and off, and every
    # one of them again at rdo_cg = 0 with the TU zero-out on
    cg = [c for c in RICH_CASES if c.rdo_cg]
    assert len(cg) >= 16 and {(c.w, c.h, c.bd) for c in cg} == {(w, h, bd) for (w, h) in util.SIZES for bd in (8, 10)} and {c.qp for c in cg} == {22, 27}
    assert {c.content for c in cg} == {"warp8", "warp16", "warp32", "b-mix16"} and {c.rdo_cg for c in cg} == {2, 5, 8} and {c.rdo_zero for c in cg} == {0, 1}
    assert all(6 <= c.noise >> (c.bd - 8) <= 8 for c in cg)
    assert {c._replace(id="") for c in RICH_CASES if not c.rdo_cg} == {c._replace(id="", rdo_cg=0, rdo_zero=1) for c in cg}
    assert sum(1 for c in INTER_CASES if c.rdo_cg and c not in RICH_CASES) == 2
    assert all(abs(int(v)) <= 56 for c in INTER_CASES if c.centres == "corners" for k in util.inter_case_centres(c, 1) for v in k.ravel())
    assert any(abs(int(v)) == 56 for c in INTER_CASES if c.centres == "corners" for k in util.inter_case_centres(c, 1) for v in k.ravel())


# ================================================================ what the MODEL reached
def test_coverage_of_the_model_over_the_cases():
    """counted on the model's own output.  `real`: the cases that run at the lambda of their QP"""
    total, real = collections.Counter(), collections.Counter()
    for c in INTER_CASES:
        inter_case_want(c)
        for k, v in INTER_COVERAGE[c.id].items():
            total[k] += v
            if c.lam is None:
                real[k] += v
    for n in (32, 16, 8):
        assert real["leaf", n] > 0
    assert real["invalid node"] > 0
    for k in range(9):
        assert real["half", k] > 0 and real["quarter", k] > 0, k
    assert real["ring tie", "ring only"] > 0           # two ring positions at the same lowest cost, the centre not among them, at a real lambda
    assert real["ring tie"] > real["ring tie", "ring only"]            # ... and ties of the centre with a ring position
    assert real["B key tie"] > 0
    # at a real lambda they are list 0 == list 1; at lambda_sad_q4 = 0 a tie with the bi key is one of all three keys
    assert real["B key tie", (M.L0, M.L1)] > 0 and total["B key tie", (M.L0, M.L1, M.BI)] > 0
    # list 1 == both lists with list 0 dearer: the two cases tools/find_b_key_tie.py found (lambda_sad_q4 16 and 32); the first of equal keys is list 1
    assert total["B key tie", (M.L1, M.BI)] >= 2
    for m in (M.L0, M.L1, M.BI):
        assert real["B mode", m] > 0
    assert real["zero-out", "zeroed"] > 0 and real["zero-out", "kept"] > 0
    assert real["slice removed the winner"] > 0        # a ring candidate cheaper than the winner, whose rows leave the slice
    # whole == split needs (SATD difference) x 16 == lambda x (bits difference + 14): it occurs at lambda_sad_q4 = 0 only
    assert total["whole == split"] > 0 and real["whole == split"] == 0
    print(sorted(total.items(), key=str))


def test_coverage_of_the_group_drop_and_the_zero_out_on_rich_residual():
    """counted on the model's own output: conditions on the case set (util.RICH_PICTURES, seeds chosen with the model), not tolerances"""
    cg, rz, pins = collections.Counter(), collections.Counter(), collections.Counter()
    for c in INTER_CASES:
        inter_case_want(c)
        for k, v in INTER_COVERAGE[c.id].items():
            if c.rdo_cg:
                cg[k] += v
                if isinstance(k, tuple) and k[0] == "group":
                    cg[k + (c.bd,)] += v
                    cg[k[2]] += v
            if c.rdo_zero and c in RICH_CASES:
                rz[k] += v
            if c.rdo_zero and c.lam is None:
                rz["tie at the QP's own lambda"] += v if k == "zero-out tie" else 0
            if c.rdo_zero and k == "zero-out tie":
                rz["tie, all cases"] += v
    for c in INTER_PINS.values():
        inter_case_want(c)
        pins.update(INTER_COVERAGE[c.id])
    assert cg["dropped"] >= 200 and cg["kept"] >= 200
    for bd in (8, 10):
        for where in (("luma", 8), ("luma", 16), ("luma", 32), ("chroma", 4), ("chroma", 8), ("chroma", 16)):
            assert cg["group", where, "dropped", bd] > 0 and cg["group", where, "kept", bd] > 0, (where, bd)
    assert cg["group drop emptied a TU"] >= 10
    assert cg["group drop thinned, zero-out removed"] >= 1
    assert pins["group equality"] >= 4                                      # 16 D == threshold: the four hand-worked pins
    assert rz["zero-out", "zeroed"] + rz["zero-out", "kept"] >= 300         # TUs that reach the TU zero-out with a level, among the rich cases alone
    assert rz["tie, all cases"] >= 2 and rz["tie at the QP's own lambda"] >= 1         # jz == jc: what holds `jz <= jc`
    print(sorted(cg.items(), key=str), sorted(rz.items(), key=str))


@pytest.mark.parametrize("c", SATD_ROUNDING_CASES, ids=[c.id for c in SATD_ROUNDING_CASES])
def test_the_rounding_of_the_satd_per_tile_decides(monkeypatch, c):
    """the rule is (sum + 2) >> 2 per 8x8 tile.  Tile sums are even, so a CU with k tiles of sum = 2 mod 4 costs floor(k / 2) more than with one rounding of the CU's sum: at most
    2 per 16x16 and 8 per 32x32.  That moves a decision only where two costs lie this close.  In these cases the MODEL ITSELF, with one rounding per CU in its place, decides
    otherwise: an implementation that rounds per CU cannot equal the model on them (test_model_oracle_and_stepped_kernel_agree and the device file run them)"""
    want = inter_case_want(c)[0]

    def once_per_cu(diff):
        d = np.asarray(diff, np.int64)
        return (sum(int(np.abs(M.H8 @ d[y:y + 8, x:x + 8] @ M.H8.T).sum()) for y in range(0, d.shape[0], 8) for x in range(0, d.shape[1], 8)) + 2) >> 2
    monkeypatch.setattr(M, "satd", once_per_cu)
    counted = INTER_COVERAGE[c.id]
    other = inter_case_want.__wrapped__(c)[0]
    INTER_COVERAGE[c.id] = counted                             # (the coverage count is of the model as it is)
    assert any(not np.array_equal(want.cu[f], other.cu[f]) for f in ("log2_size", "mvx", "mvy", "intra_mode", "flags"))


# ================================================================ motion-constrained slices: no footprint leaves the rows
@pytest.mark.parametrize("c", [c for c in INTER_CASES if c.mc != (0, 0)], ids=[c.id for c in INTER_CASES if c.mc != (0, 0)])
def test_no_footprint_leaves_the_slice(emu, c):
    """independent of the model: the records of the oracle and of the stepped kernel, by the footprint function of tests/test_sliced_cpu.py; and the
    constraint binds: the same case without it codes other vectors"""
    free = c._replace(mc=(0, 0))
    for run in (run_inter_case(O, c), run_inter_case(emu, c)):
        for (by, bx), r in np.ndenumerate(run.cu):
            n = 1 << int(r["log2_size"])
            assert mv_rows_ok((by * 8) & ~(n - 1), n, int(r["mvy"]), c.h, *c.mc), (bx, by, r)
    assert not np.array_equal(run_inter_case(O, free).cu["mvy"], run_inter_case(O, c).cu["mvy"])
