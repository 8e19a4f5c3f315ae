"""CPU: everything the inter CTU program (`inter_ctu_program`: `k_inter_ctu`, `k_inter_ctu_b`) decides after the integer search — quadtree, half- and
quarter-sample vectors, the list choice of B pictures, the RD zero-out, records, levels, reconstruction, rate estimate — held to tests/hevc_inter_cu.py,
a brute-force numpy model written from DESIGN.md §6 ("Decision rules of the inter CTU program, in words") and not from oracle/hevc_oracle.c or the kernel.
The oracle is the kernel's scalar twin (same ring table, same packed key, same bottom-up pass): a rule both have wrong yields a valid stream that decodes to
the encoder's own reconstruction and only costs bits or quality.

First hand-worked pictures, each through the model, the oracle and the stepped kernel in three lane orders.  Then model == oracle == stepped kernel on
util.INTER_CASES (shared with tests/test_gpu_inter_cu_independent.py, which runs them on the device without the oracle), what the MODEL reached over
them, and the footprint property of motion-constrained slices."""
import collections

import numpy as np
import pytest

from oracle import oracle as O
from tests import hevc_analysis as A
from tests import hevc_inter_cu as M
from tests import util
from tests.test_sliced_cpu import mv_rows_ok
from tests.util import INTER_CASES, INTER_COVERAGE, INTER_PINS, PIN_B_MVS, PIN_MVS, PIN_SPLIT_MVS, SATD_ROUNDING_CASES, inter_case_params, inter_case_want, inter_diff, run_inter_case

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


# ================================================================ model == oracle == stepped kernel
@pytest.mark.parametrize("c", INTER_CASES, ids=[c.id for c in INTER_CASES])
def test_model_oracle_and_stepped_kernel_agree(emu, c):
    want, me, _ = inter_case_want(c)
    orc, got = run_inter_case(O, c), run_inter_case(emu, c)
    for l, m in enumerate(me):
        for name, a in (("oracle", orc), ("stepped kernel", got)):
            t = a.me if len(me) == 1 else a.me[l]
            assert np.array_equal(t, m), f"integer table, list {l}: {name} != model: " + util.first_diff(t, m)
    d = inter_diff(want, orc, decisions_only=c.rdo_cg > 0)
    assert not d, "oracle != model: " + d
    d = inter_diff(want, got, decisions_only=c.rdo_cg > 0)
    assert not d, "stepped kernel != model: " + d


def test_the_cases_are_the_ones_asked_for():
    plain = {(c.w, c.h, c.bd, c.R, c.qp, c.rdo_zero) for c in INTER_CASES if c.content.startswith("warp") and c.lam is None and c.mc == (0, 0) and not c.rdo_cg}
    assert plain >= {(w, h, bd, R, qp, rz) for (w, h) in util.SIZES for bd in (8, 10) for R in (8, 15) for qp in (22, 32, 42) for rz in (0, 1)}
    assert {c.mc for c in INTER_CASES} == {(0, 0), (1, 0), (0, 1), (1, 1)} and any(c.pre_search for c in INTER_CASES) and any(c.centres == "corners" for c in INTER_CASES)
    assert any(c.lam and c.lam[0] == 0 for c in INTER_CASES) and any(c.content.startswith("b-") for c in INTER_CASES)
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
    # at a real lambda they are list 0 == list 1; a tie with the bi key occurs at lambda_sad_q4 = 0 only, as one of all three keys
    assert real["B key tie", (M.L0, M.L1)] > 0 and total["B key tie", (M.L0, M.L1, M.BI)] > 0
    for m in (M.L0, M.L1, M.BI):
        assert real["B mode", m] > 0
    assert real["zero-out", "zeroed"] > 0 and real["zero-out", "kept"] > 0
    assert real["slice removed the winner"] > 0        # a ring candidate cheaper than the winner, whose rows leave the slice
    # whole == split needs (SATD difference) x 16 == lambda x (bits difference + 14): it occurs at lambda_sad_q4 = 0 only
    assert total["whole == split"] > 0 and real["whole == split"] == 0
    print(sorted(total.items(), key=str))


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
