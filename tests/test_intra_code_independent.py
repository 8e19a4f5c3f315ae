"""CPU: the intra CODE stage (every IDR picture), the NxN trial and the intra second pass of P pictures held to tests/hevc_intra_code.py, a brute-force
numpy model written from DESIGN.md §6 ("Decision rules of the intra code stage, the NxN trial and the intra second pass, in words") and H.265 6.4.1 /
8.4.2 / 8.4.4.2 / 8.6, not from oracle/hevc_oracle.c or kernels/intra.h.  The oracle's intra_code_ctu / intra_in_p_pass are the kernels' scalar twins
(same keys, same park-and-restore, same modular correction of the estimate): a rule both have wrong — an intra rounding swapped for the inter dead zone,
a candidate list that forgets the left CTU, an NxN tie given to NxN, an activity that keeps its DC term, a round that admits a CTU whose neighbour never
ran — yields valid streams that decode to the encoder's own reconstruction and passes every parity, syntax, reconstruction and decoder test.  Here a
third statement must agree with both, exactly: records, levels, reconstruction and rate estimate.

First the model is pinned by answers worked out by hand, each also through the oracle and the stepped kernel source (sequential, reversed and random
lane order, the last over random initial LDS).  Then model == oracle == stepped kernel on the cases of tests/util.py, a coverage count shows what the
MODEL reached, and two binding tests show that the candidate list of the code stage and the DC term of the activity decide something in these cases.
tests/test_gpu_intra_code_independent.py runs the device entries against the model."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import hevc_intra_code as M
from tests import hevc_intra_plan as P
from tests import util
from tests.util import (CODE_CASES, CODE_COVERAGE, CODE_SIGN_HIDE_CASES, P_CODE_CASES, P_CODE_SIGN_HIDE_CASES, code_case_params, code_case_want, inter_diff,
                        p_code_case_params, p_code_case_pictures, p_code_case_want, plan_case_source)

LAM_SAD, LAM = 38, 92            # QP 22 at 8 bit (mihevc_cost_params_for_qp), used where a hand-worked case needs numbers
LANE_ORDERS = (("0", None), ("1", None), ("2", "11"))          # sequential, reversed, random lane order (the last over random initial LDS)


@pytest.fixture(scope="module")
def emu():
    return util.StageApi(util.stepped_library(), "emu_")


@pytest.fixture(scope="module")
def emu_sdh():
    return util.StageApi(util.stepped_library(), "emu_", sign_hide=1)


def in_lane_orders(monkeypatch, run, want, what):
    """run(): one pass of the stepped kernel source -> O.Analysis; held to the model's result in the three lane orders"""
    for order, fill in LANE_ORDERS:
        monkeypatch.setenv("EMU_ORDER", order)
        if fill:
            monkeypatch.setenv("EMU_SHARED_FILL", fill)
        d = inter_diff(want, run())
        assert not d, f"{what}: stepped kernel (lane order {order}) != model: {d}"
    monkeypatch.delenv("EMU_SHARED_FILL", raising=False)


def held_i(emu, monkeypatch, planes, bd=8, qp=22, nxn=1, chroma_modes=1, tiles=(1, 1), **lambdas):
    """the model's result of a hand-made I picture (and the model's plan of it), after the oracle AND the stepped kernel source have been held to it"""
    prm, cp = util.params_pair(qp, bd, 8, intra_nxn=nxn, chroma_modes=chroma_modes, tile_cols=tiles[0], tile_rows=tiles[1], **lambdas)
    plan = P.plan_picture(planes, bd, cp.qp, cp.qp_c, cp.lambda_sad_q4, cp.lambda_q4, tiles[0], tiles[1], chroma_modes)
    want = M.code_picture(planes, plan, util.model_params(cp))
    src = O.Frame(*planes)
    d = inter_diff(want, O.analyze_intra(src, prm))
    assert not d, "oracle != model: " + d
    in_lane_orders(monkeypatch, lambda: emu.intra(src, cp), want, "hand-made picture")
    return want, plan


def held_p(emu, monkeypatch, cur, ref, prm, cp, **switches):
    want = M.second_pass(util.planes3(cur), util.planes3(ref), util.model_params(cp), **switches)
    d = inter_diff(want, O.analyze_inter(cur, ref, prm, dump_me=True))
    assert not d, "oracle != model: " + d
    in_lane_orders(monkeypatch, lambda: emu.inter(cur, ref, cp), want, "hand-made pair")
    return want


def quadrant_picture(w, h, bd=8):
    """every 8x8 cell: its four 4x4 quadrants are stripes along four directions — down the columns, along the rows, along x + y and along x - y; chroma is
    striped along a fifth direction, so that the plan's chroma mode is its own"""
    a = np.array(util.STRIPE) << (bd - 8)
    yy, xx = np.mgrid[0:h, 0:w]
    qx, qy = (xx >> 2) & 1, (yy >> 2) & 1
    y = np.where(qy == 0, np.where(qx == 0, a[xx % 8], a[(yy + 3) % 8]), np.where(qx == 0, a[(xx + yy) % 8], a[(xx - yy) % 8]))
    c = a[(xx[:h // 2, :w // 2] + 2 * yy[:h // 2, :w // 2]) % 8] // 4 + (96 << (bd - 8))
    return y, c, c.T.copy()


# ================================================================ hand-worked answers
def test_flat_picture_codes_nothing_and_costs_its_bits(emu, monkeypatch):
    """Every prediction of a flat picture is exact: no level anywhere, SSE 0.  Every CTU is one 32x32 CU in planar mode (the plan's pins), whose list is
    {planar, DC, 26} at the origin (both neighbours DC) and {planar, DC, 26} again where the left CTU answers planar and the CTU above is never asked: 2 bits
    of mode, 1 of flags, 1.5 of chroma mode and cbfs = 72 sixteenths; J = (lambda x 72) >> 4, J_ctu = lambda + J, and the estimate is 128 per CU."""
    v = np.full((64, 64), 128)
    r, plan = held_i(emu, monkeypatch, (v, v[::2, ::2], v[::2, ::2]))
    assert sorted(r.cus) == [(0, 0), (0, 32), (32, 0), (32, 32)]
    for k in r.cus.values():
        assert (k["size"], k["mode"], k["cmode"], k["cand"], k["sse"], k["bits"], k["total_bits"], k["j"]) == (32, 0, 0, [0, 1, 26], 0, [0, 0, 0], 72, (LAM * 72) >> 4)
    assert not any(c.any() for c in r.coef) and all((p == 128).all() for p in r.rec)
    assert r.est == 4 * 128 and all(t == {"j_ctu": LAM + ((LAM * 72) >> 4), "est": 128} for t in r.ctus.values())
    assert (r.cu["flags"] == 0).all() and (r.cu["log2_size"] == 5).all() and (r.cu["qp"] == 22).all() and not r.cu["intra_mode"].any()


def test_the_left_ctu_feeds_the_list_and_a_tile_edge_does_not(emu, monkeypatch):
    """Column stripes: below the first CTU row the plan (on the source) finds mode 26 exact and makes every CTU there one 32x32 CU in mode 26 (the plan's
    pins).  CTU (1, 1): A = the left CTU's record = 26, B = DC because it lies in the CTU above: {26, DC, planar}, 26 is the FIRST candidate: 2 bits of
    mode, 72 sixteenths before the levels.  The plan's own list asked nobody outside the CTU: {planar, DC, 26}, 3 bits.  With two tile columns CTU (1, 1) is
    a tile's first column: A = DC, {planar, DC, 26}, 26 is the third: 3 bits, 88 — its row above is still there, so the plan keeps the mode.  (The row above
    is the first CTU row's RECONSTRUCTION here, not the source: the prediction is no longer exact and levels are coded, which J counts on top.)"""
    src = plan_case_source("stripes", 64, 64, 8)
    r, plan = held_i(emu, monkeypatch, util.planes3(src))
    k = r.cus[32, 32]
    assert (k["size"], k["mode"], k["cand"], k["total_bits"] - sum(k["bits"])) == (32, 26, [26, 1, 0], 72) and k["j"] == (k["sse"] << 4) + ((LAM * k["total_bits"]) >> 4)
    assert M.IntraCodeModel(util.planes3(src), util.model_params(util.params_pair(22, 8, 8)[1])).plan_list(plan[3], 0) == [0, 1, 26]
    k = r.cus[0, 32]                                                                          # the picture's first column: nobody to the left
    assert (k["mode"], k["cand"], k["total_bits"] - sum(k["bits"])) == (26, [0, 1, 26], 88)
    t, _ = held_i(emu, monkeypatch, util.planes3(src), tiles=(2, 1))
    k = t.cus[32, 32]
    assert (k["size"], k["mode"], k["cand"], k["total_bits"] - sum(k["bits"])) == (32, 26, [0, 1, 26], 88) and k["j"] == (k["sse"] << 4) + ((LAM * k["total_bits"]) >> 4)


def test_four_directions_in_one_cu_make_nxn_win(emu, monkeypatch):
    """24x24: the 8x8 nodes along the right and bottom edge are leaves whatever they cost (their 16x16 does not fit the picture).  The CU at (16, 0) has four
    quadrants striped along four directions, which no single mode predicts: the trial runs (the 2Nx2N coding leaves luma levels), the four PUs pick four
    DIFFERENT modes and NxN is cheaper.  PU 1 (20, 0) has no bottom-left — (19, 4..7) lies in PU 2, coded after it — and PU 3 (20, 4) no top-right, which is
    the next CU: both see substituted samples.  Chroma is coded with PU 0's mode, which the record's chroma_mode reports, whatever the plan chose."""
    planes = quadrant_picture(24, 24)
    r, plan = held_i(emu, monkeypatch, planes)
    k = r.cus[16, 0]
    n = k["nxn"]
    assert n["kept"] and n["j_nxn"] < n["j_2nx2n"] and k["j"] == n["j_nxn"] and len(set(n["modes"])) == 4
    rec = r.cu[0, 2]
    assert rec["flags"] & 16 and rec["intra_mode"].tolist() == n["modes"] and rec["chroma_mode"] == n["modes"][0] != plan[0]["cmode"][P.NODE_AT[(16, 0, 8)]]
    assert rec["cbf_y4"] == 15 and rec["flags"] & 2 and not rec["mvx"] and not rec["mvy"] and not rec["pad"].any()
    assert all(len(t) == 35 for t in n["tables"]) and [t.index(min(t)) for t in n["tables"]] == n["modes"]
    assert r.cov["PU without bottom-left", 1] >= 1 and r.cov["PU without top-right", 3] >= 1
    m = M.IntraCodeModel(planes, util.model_params(util.params_pair(22, 8, 8)[1]))
    _, avail = m.references(r.rec, 0, 20, 0, 4, 20, 0)          # PU 1 of that CU: row -1 is outside the picture, (19, 0..3) is PU 0, (19, 4..7) is PU 2
    assert avail.tolist() == [False] * 4 + [True] * 4 + [False] * 9
    _, avail = m.references(r.rec, 0, 20, 4, 4, 20, 4)          # PU 3: left is PU 2, below it the next CU; above PU 1, then (24..27, 3): outside the picture
    assert avail.tolist() == [False] * 4 + [True] * 9 + [False] * 4
    _, avail = m.references(r.rec, 0, 20, 20, 4, 20, 20)        # PU 3 of the CU at (16, 16): the same, z-order alone
    assert avail.tolist() == [False] * 4 + [True] * 9 + [False] * 4
    _, avail = m.references(r.rec, 1, 8, 8, 4, 16, 16)          # the chroma block of the CU at (16, 16) counts by the CU's address: 8 left (4 of them below the picture), corner, 4 above
    assert avail.tolist() == [False] * 4 + [True] * 9 + [False] * 4


def test_nxn_at_equal_cost_stays_2nx2n(emu, monkeypatch):
    """The same picture where J_nxn EQUALS J_2Nx2N.  No lambda_q4 produces it at QP 22 .. 37: in all its CUs NxN has the smaller SSE and no more bits, so it wins at
    every lambda (searched with the model alone over lambda_q4 < 200000).  So lambda_q4 = 0, where J is 16 SSE: at QP 0 the CUs at (16, 8) and (16, 16) rebuild
    with a squared error of 4 both ways: 64 against 64, and the 2Nx2N coding stays; the CU at (8, 16), 5 against 3, goes NxN."""
    r, _ = held_i(emu, monkeypatch, quadrant_picture(24, 24), qp=0, lambda_q4=0)
    for xy in ((16, 8), (16, 16)):
        n = r.cus[xy]["nxn"]
        assert n["j_nxn"] == n["j_2nx2n"] == 64 and not n["kept"] and not r.cu[xy[1] >> 3, xy[0] >> 3]["flags"] & 16
    n = r.cus[8, 16]["nxn"]
    assert (n["j_2nx2n"], n["j_nxn"], n["kept"]) == (80, 48, True) and r.cu[2, 1]["flags"] & 16
    assert r.cov["nxn", "tie"] >= 2


def test_a_cu_without_a_luma_level_is_not_tried(emu, monkeypatch):
    """flat luma under textured chroma: the 2Nx2N coding of the forced 8x8 leaves has chroma levels and no luma level: no trial, no NxN record"""
    rng = np.random.default_rng(5)
    y = np.full((24, 24), 128)
    r, _ = held_i(emu, monkeypatch, (y, rng.integers(40, 220, (12, 12)), rng.integers(40, 220, (12, 12))))
    assert r.cov["nxn", "not tried, chroma has a level"] >= 3 and not r.cov["nxn", "kept"] and not r.cov["nxn", "refused"]
    assert not (r.cu["flags"] & 16).any() and (r.cu["flags"] & 12).any() and not (r.cu["flags"] & 2).any()


def test_the_schedule_on_hand_made_maps():
    """round 0: candidates with no candidate to the left, top-left, top, top-right; round 1: the others whose candidate neighbours were ALL in round 0;
    -1: never tried; -2: no candidate"""
    ones = M.schedule(np.ones((3, 4), bool))
    assert ones.tolist() == [[0, 1, -1, -1], [-1, -1, -1, -1], [-1, -1, -1, -1]]          # only CTUs (0, 0) and (1, 0)
    yy, xx = np.mgrid[0:4, 0:5]
    checker = M.schedule((xx + yy) % 2 == 0)
    # row 0: nobody around; row 1: top-left and top-right are candidates of round 0; row 2: theirs are of round 1: never; row 3 likewise
    assert checker.tolist() == [[0, -2, 0, -2, 0], [-2, 1, -2, 1, -2], [-1, -2, -1, -2, -1], [-2, -1, -2, -1, -2]]
    row = np.zeros((3, 5), bool)
    row[1] = True
    assert M.schedule(row).tolist() == [[-2] * 5, [0, 1, -1, -1, -1], [-2] * 5]
    col = np.zeros((4, 3), bool)
    col[:, 1] = True
    assert M.schedule(col).tolist() == [[-2, 0, -2], [-2, 1, -2], [-2, -1, -2], [-2, -1, -2]]
    # the top-right neighbour counts: (0, 1) under a candidate at (1, 0)
    tr = np.zeros((2, 2), bool)
    tr[0, 1] = tr[1, 0] = True
    assert M.schedule(tr).tolist() == [[-2, 0], [1, -2]]


def test_an_unrelated_picture_converts_two_ctus_at_most(emu, monkeypatch):
    """a P picture that has nothing to do with its reference (a black one: the inter cost holds the mean that the activity leaves out): EVERY CTU is a
    candidate, and of a connected field of candidates only its first CTU runs in round 0 and the one to its right in round 1: the other 13 stay inter,
    however bad"""
    c = next(k for k in P_CODE_CASES if k.content == "unrelated")
    prm, cp = p_code_case_params(c)
    cur, ref = p_code_case_pictures(c)
    r = held_p(emu, monkeypatch, cur, ref, prm, cp)
    assert all(t["candidate"] for t in r.ctus.values()) and [t["round"] for t in r.ctus.values()] == [0, 1] + [-1] * 13
    assert r.ctus[0]["replaced"] and r.ctus[1]["replaced"]
    intra = (r.cu["flags"] & 1) == 0
    assert intra[:4, :8].all() and intra.sum() == 32, "CTUs (0, 0) and (1, 0) go intra and nothing else does"


def checker_pair(mean, amp, w=64, h=32):
    """mean +- amp in a checkerboard against a flat reference of 128: with lambda_sad_q4 = 0 the cost of a CTU is its SATD alone.  An 8x8
    tile of the difference has two coefficients, 64 amp at the highest frequency and 64 (mean - 128) at DC: SATD = (64 amp + 64 |mean - 128| + 2) >> 2 per
    tile, and the source tile's activity is (64 amp + 2) >> 2 = 16 amp"""
    yy, xx = np.mgrid[0:h, 0:w]
    c = np.full((h // 2, w // 2), 128)
    return O.Frame(mean + amp * (1 - 2 * ((xx + yy) & 1)), c, c), O.Frame(np.full((h, w), 128), c, c)


def test_the_candidate_tests_at_their_boundaries_on_pictures(emu, monkeypatch):
    """128 +- 40: cost = 16 tiles x 640 << 4 = 163840 = act << 4 EXACTLY: no candidate, the picture stays inter — though the CTU, tried, would have been
    replaced (the model with one more unit of cost says so: a `>=` in the second test changes this picture).  129 +- 15: (960 + 64 + 2) >> 2 = 256 per
    tile, cost = (256 x 16) << 4 EXACTLY, activity 240 per tile: a candidate, tried and replaced.  128 +- 16: both equalities at once: no candidate."""
    prm, cp = util.params_pair(22, 8, 8, intra_in_p=1, chroma_modes=1, intra_nxn=1, lambda_sad_q4=0)
    cur, ref = checker_pair(128, 40)
    r = held_p(emu, monkeypatch, cur, ref, prm, cp)
    assert [(t["cost"], t["act"] << 4, t["candidate"]) for t in r.ctus.values()] == [(163840, 163840, False)] * 2 and (r.cu["flags"] & 1).all()
    above = M.second_pass(util.planes3(cur), util.planes3(ref), util.model_params(cp), planted={0: {"cost": 163841}})
    assert above.ctus[0]["candidate"] and above.ctus[0]["replaced"] and not above.same(r)
    cur, ref = checker_pair(129, 15)
    r = held_p(emu, monkeypatch, cur, ref, prm, cp)
    assert [(t["cost"], (256 * t["tiles"]) << 4, t["act"], t["candidate"]) for t in r.ctus.values()] == [(65536, 65536, 3840, True)] * 2
    assert [t["round"] for t in r.ctus.values()] == [0, 1] and r.ctus[0]["replaced"] and not (r.cu["flags"][:, :4] & 1).any()
    below = M.second_pass(util.planes3(cur), util.planes3(ref), util.model_params(cp), planted={0: {"cost": 65535}})
    assert not below.ctus[0]["candidate"] and not below.same(r)
    cur, ref = checker_pair(128, 16)
    r = held_p(emu, monkeypatch, cur, ref, prm, cp)
    assert [(t["cost"], t["act"] << 4, t["candidate"]) for t in r.ctus.values()] == [(65536, 65536, False)] * 2 and (r.cu["flags"] & 1).all()
    assert r.cov["candidate", "cost == 4 per sample"] == 2 and r.cov["candidate", "cost == activity"] == 2


def flat_step_pair(w=64, h=32):
    """flat 144 against a flat reference of 128: the difference is 16 everywhere, one DC coefficient per block, which every QP used here rebuilds exactly"""
    c = np.full((h // 2, w // 2), 128)
    return O.Frame(np.full((h, w), 144), c, c), O.Frame(np.full((h, w), 128), c, c)


def test_intra_at_equal_cost_stays_inter(emu, monkeypatch):
    """J_ctu < jinter replaces; EQUAL does not.  Flat 144 against flat 128 at both lambdas 0: a tile's SATD is (64 x 16 + 2) >> 2 = 256, so cost = (256 x 16) << 4
    and the activity is 0: both CTUs are candidates, round 0 and round 1, and both are tried.  The inter version rebuilds the step exactly (SSE 0) and so
    does the intra one (CTU 0 predicts 128 from nothing, CTU 1 predicts 144 from its left neighbour): with lambda_q4 = 0, J_ctu == jinter == 0, and the
    inter version stays: every record inter, the estimate the inter one.  With `>=` turned into `>` both CTUs would go intra."""
    cur, ref = flat_step_pair()
    for qp in (22, 32):
        prm, cp = util.params_pair(qp, 8, 8, intra_in_p=1, chroma_modes=1, intra_nxn=1, lambda_sad_q4=0, lambda_q4=0)
        r = held_p(emu, monkeypatch, cur, ref, prm, cp)
        assert [(t["cost"], t["act"], t["candidate"], t["round"]) for t in r.ctus.values()] == [(65536, 0, True, 0), (65536, 0, True, 1)]
        for t in r.ctus.values():
            assert t["j_ctu"] == t["jinter"] == 0 and not t["replaced"] and t["est_intra"] != t["est_inter"]
        assert (r.cu["flags"] & 1).all() and r.est == r.inter.est == sum(t["est_inter"] for t in r.ctus.values())
        assert all((p == v).all() for p, v in zip(r.rec, (144, 128, 128))) and r.cov["tried", "j_ctu == jinter"] == 2 and r.cov["tried", "kept inter"] == 2


def test_the_candidate_tests_at_their_boundaries():
    """cost >= (256 x tiles) << 4 AND cost > act << 4: exactly 4 per sample passes, equal to the activity does not.  The pictures of the parametrised cases
    reach neither equality (the hand-made checkerboards above do); here the sums are planted in the model's twin: a flat pair, CTU 0 of 16 tiles."""
    cur, ref = util.flat_pair(64, 32, 8)
    _, cp = util.params_pair(27, 8, 8, intra_in_p=1, chroma_modes=1)
    four = (256 * 16) << 4
    for cost, act, want in ((four, 0, True), (four - 1, 0, False), (80000 << 4, 80000, False), ((80000 << 4) + 1, 80000, True), (four, 4096, False), (four + 1, 4096, True)):
        r = M.second_pass(util.planes3(cur), util.planes3(ref), util.model_params(cp), planted={0: {"cost": cost, "act": act, "tiles": 16}})
        assert r.ctus[0]["candidate"] == want and (r.ctus[0]["round"] == 0) == want, (cost, act)
        assert r.ctus[1]["candidate"] is False and r.ctus[1]["cost"] == 2 * cp.lambda_sad_q4        # the flat pair's own sums: one 32x32 CU, zero vector, 2 bits
    assert hadamard_ac_by_hand()


def hadamard_ac_by_hand():
    """the activity of a tile: a constant tile has none (its only coefficient is the DC one); a tile of +-1 in a checkerboard has one coefficient of 64 away
    from DC: (64 + 2) >> 2 = 16; with a mean of 100 on top still 16 (the DC coefficient is the only one the mean moves)"""
    yy, xx = np.mgrid[0:8, 0:8]
    chk = 1 - 2 * ((xx + yy) & 1)
    return M.hadamard_ac(np.full((8, 8), 77)) == 0 and M.hadamard_ac(chk) == 16 and M.hadamard_ac(chk + 100) == 16


# ================================================================ model == oracle == stepped kernel on the cases of tests/util.py
@pytest.mark.parametrize("c", CODE_CASES, ids=[c.id for c in CODE_CASES])
def test_i_picture_model_oracle_and_stepped_kernel_agree(emu, monkeypatch, c):
    want = code_case_want(c)
    prm, cp = code_case_params(c)
    src = plan_case_source(c.plan.content, c.plan.w, c.plan.h, c.plan.bd)
    d = inter_diff(want, O.analyze_intra(src, prm))
    assert not d, "oracle != model: " + d + explain(want)
    in_lane_orders(monkeypatch, lambda: emu.intra(src, cp), want, c.id)


@pytest.mark.parametrize("c", P_CODE_CASES, ids=[c.id for c in P_CODE_CASES])
def test_p_picture_model_oracle_and_stepped_kernel_agree(emu, monkeypatch, c):
    want = p_code_case_want(c)
    prm, cp = p_code_case_params(c)
    cur, ref = p_code_case_pictures(c)
    d = inter_diff(want, O.analyze_inter(cur, ref, prm, dump_me=True))
    assert not d, "oracle != model: " + d + explain(want)
    in_lane_orders(monkeypatch, lambda: emu.inter(cur, ref, cp), want, c.id)


@pytest.mark.parametrize("c", CODE_SIGN_HIDE_CASES + P_CODE_SIGN_HIDE_CASES, ids=[c.id for c in CODE_SIGN_HIDE_CASES + P_CODE_SIGN_HIDE_CASES])
def test_sign_hiding_model_and_stepped_kernel_agree(emu_sdh, monkeypatch, c):
    """sign data hiding in intra blocks: the scan follows (block size, plane, mode); NxN on.  The oracle has no sign hiding: model against the stepped kernels"""
    if isinstance(c, util.CodeCase):
        want, (_, cp), src = code_case_want(c), code_case_params(c), plan_case_source(c.plan.content, c.plan.w, c.plan.h, c.plan.bd)
        plain = code_case_want(c._replace(sign_hide=0))
        in_lane_orders(monkeypatch, lambda: emu_sdh.intra(src, cp), want, c.id)
    else:
        want, (_, cp), (cur, ref) = p_code_case_want(c), p_code_case_params(c), p_code_case_pictures(c)
        plain = p_code_case_want(c._replace(sign_hide=0))
        in_lane_orders(monkeypatch, lambda: emu_sdh.inter(cur, ref, cp), want, c.id)
        assert any(t.get("replaced") for t in want.ctus.values())
    assert not want.same(plain) and (want.cu["flags"] & 16).any(), "sign hiding changed nothing, or no NxN CU: the case does not test what it is for"


def explain(want):
    """the model's own account of its CTUs, for a failure message"""
    return "; model: " + ", ".join(f"CTU {k}: {t}" for k, t in want.ctus.items() if t.get("round", 0) > -2)[:2000]


# ================================================================ what the model reached
def test_the_model_alone_reaches_every_rule():
    for c in CODE_CASES:
        code_case_want(c)
    for c in P_CODE_CASES:
        p_code_case_want(c)
    cov = CODE_COVERAGE
    want = [("nxn", k) for k in ("kept", "refused", "not tried", "tie")] + [("PU with an unavailable sample", k) for k in range(4)]
    want += [("PU without bottom-left", 1), ("PU without top-right", 3)]
    want += [("PU list", "left", "a PU of an NxN CU"), ("PU list", "above", "a PU of an NxN CU"), ("PU list", "left", "the left CTU: a PU of an NxN CU"), ("PU list", "left", "a PU of the same CU")]
    want += [("list", "left", k) for k in ("the left CTU: a 2Nx2N CU", "the left CTU: a PU of an NxN CU", "the left CTU: an inter record", "a tile's edge", "the picture's edge")]
    want += [("list", "above", "the CTU above")]
    want += [("candidate", k) for k in ("refused by the first test", "refused by the second test", "yes")] + [("round", k) for k in ("0", "1", "never", "no candidate")]
    want += [("tried", "replaced"), ("tried", "kept inter"), "replaced CTU with an NxN CU", "round-1 CTU next to a replaced round-0 CTU"]
    print({str(k): cov[k] for k in want + [("candidate", "cost == 4 per sample"), ("candidate", "cost == activity"), ("tried", "j_ctu == jinter")]})
    missing = [k for k in want if not cov[k]]
    assert not missing, missing
    # NOT produced by any picture of these cases: the two equalities of the candidate test (the hand-made checkerboards of
    # test_the_candidate_tests_at_their_boundaries_on_pictures hold them) and J_ctu == jinter (test_intra_at_equal_cost_stays_inter holds it); if one turns up, this says so
    assert not cov["candidate", "cost == 4 per sample"] and not cov["candidate", "cost == activity"] and not cov["tried", "j_ctu == jinter"]


# ================================================================ do the cases bind?
LIST_BINDING_CASES = ("136x72-10bit-qp42-cm0-nxn1", "72x104-8bit-qp22-cm1-nxn1", "72x104-8bit-qp32-cm0-nxn1", "rails-136x72-8bit-qp45-nxn1", "rails-72x104-10bit-qp45-nxn1")
ACTIVITY_BINDING_CASES = ("patched-136x72-8bit-qp27-nxn0-rz0", "patched-72x104-10bit-qp27-nxn0-rz1", "noise-136x72-8bit-qp37-nxn1-rz1")


def test_the_candidate_list_of_the_code_stage_decides():
    """The code stage's list reaches the outputs only through J (the NxN decision, the replacement decision).  In these cases the MODEL, priced with the plan's
    list in place of its own, decides otherwise: so a code stage that took the plan's list would fail them"""
    differ = [n for n in LIST_BINDING_CASES if not code_case_want(next(c for c in CODE_CASES if c.id == n), True).same(code_case_want(next(c for c in CODE_CASES if c.id == n)))]
    assert len(differ) >= 3, differ


def test_the_dc_term_of_the_activity_decides():
    """with the DC coefficient in the activity (the mean of the tile, 64 x its level) almost no CTU's cost exceeds it: the candidates change and with them the picture"""
    differ = [n for n in ACTIVITY_BINDING_CASES if not p_code_case_want(next(c for c in P_CODE_CASES if c.id == n), False, True).same(p_code_case_want(next(c for c in P_CODE_CASES if c.id == n)))]
    assert len(differ) >= 2, differ
