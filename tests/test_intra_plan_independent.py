"""CPU: the intra plan — the luma and chroma modes of all 21 quadtree nodes of every CTU and the quadtree — held to tests/hevc_intra_plan.py, a
brute-force numpy model written from DESIGN.md §6 and H.265 8.4.2 / 8.4.4.2, not from oracle/hevc_oracle.c or kernels/intra.h.  The oracle's
intra_plan_ctu is the kernel's scalar twin (same packed key, same candidate helper, same per-level RD pass): a rule both have wrong — a reference sample
wrongly judged available, a smoothing threshold off by one, a SATD that skips a tile, a tie going the other way — yields valid streams that only cost
bits and passes every parity, syntax, reconstruction and golden test.  Here a third statement must agree with both, exactly.

First the model is pinned by answers worked out by hand.  Then model == oracle (orc_intra_plan_frame) == stepped kernel source (emu_intra_plan, in
sequential, reversed and random lane order) on the cases of tests/util.py, a coverage count shows what the MODEL reached, and the code stage must carry
the plan into its CU records.  tests/test_gpu_intra_plan_independent.py runs the device entry against the model."""
import collections

import numpy as np
import pytest

from oracle import oracle as O
from tests import hevc_intra_plan as M
from tests import hevc_recon as R
from tests import util
from tests.util import PLAN_CASES, PLAN_COVERAGE, check_records_carry_the_plan, plan_case_source, plan_case_want, plan_diff

def drawn_picture(i):
    """the decoded pictures of tests/test_syntax_independent.py's hand-drawn all-modes stream"""
    def make(w, h, bd):
        from tests.test_syntax_independent import encoded
        frames, _ = O.decode(encoded("drawn-intra-224x160")[1])
        assert frames[i].shape == (h, w) and bd == 8
        return frames[i]
    return make


util.PLAN_SOURCES.update(drawn0=drawn_picture(0), drawn1=drawn_picture(1))

LAM_SAD, LAM = 38, 92            # QP 22 at 8 bit (mihevc_cost_params_for_qp), used where a hand-worked case needs numbers


def picture(y, c=None, bd=8):
    y = np.asarray(y, np.int64)
    c = np.full((y.shape[0] // 2, y.shape[1] // 2), 1 << (bd - 1), np.int64) if c is None else np.asarray(c, np.int64)
    return (y, c, c.copy())


def plan_of(planes, bd=8, qp=22, lam_sad=LAM_SAD, lam=LAM, chroma_modes=1, tiles=(1, 1), detail=None, cov=None):
    return M.plan_picture(planes, bd, qp, qp, lam_sad, lam, tiles[0], tiles[1], chroma_modes, cov, detail)


def oracle_of(planes, bd=8, qp=22, lam_sad=LAM_SAD, lam=LAM, chroma_modes=1):
    prm = O.Params(qp, qp, bd, lam_sad, lam, 8, 1, 1, 0, 0, 0, 0, chroma_modes)
    return O.intra_plan(O.Frame(*planes), prm)


LANE_ORDERS = (("0", None), ("1", None), ("2", "11"))          # sequential, reversed, random lane order (the last over random initial LDS)


@pytest.fixture(scope="module")
def emu():
    return util.StageApi(util.stepped_library(), "emu_")


def held(emu, monkeypatch, planes, bd=8, qp=22, lam_sad=LAM_SAD, lam=LAM, chroma_modes=1, detail=None):
    """the model's plan of a hand-made picture, after the oracle AND the stepped kernel source (in the three lane orders) have been held to it"""
    from hevc_amd import _lib
    want = plan_of(planes, bd, qp, lam_sad, lam, chroma_modes, detail=detail)
    got = oracle_of(planes, bd, qp, lam_sad, lam, chroma_modes)
    assert got.tobytes() == want.tobytes(), "oracle != model: " + plan_diff(got, want)
    cp = _lib.CostParams(qp, qp, bd, lam_sad, lam, 8, 1, 1, 0, 0, 0, 0, chroma_modes, 0, 0, 0)
    for order, fill in LANE_ORDERS:
        monkeypatch.setenv("EMU_ORDER", order)
        if fill:
            monkeypatch.setenv("EMU_SHARED_FILL", fill)
        got = emu.intra_plan(O.Frame(*planes), cp)
        assert got.tobytes() == want.tobytes(), f"stepped kernel (lane order {order}) != model: " + plan_diff(got, want)
    monkeypatch.delenv("EMU_SHARED_FILL", raising=False)
    return want


def satd8_by_hand(d):
    """8x8 Hadamard by its definition, entry by entry: H[i][j] = (-1)^popcount(i & j)"""
    h = [[-1 if bin(i & j).count("1") & 1 else 1 for j in range(8)] for i in range(8)]
    s = 0
    for u in range(8):
        for v in range(8):
            s += abs(sum(h[u][y] * int(d[y][x]) * h[v][x] for y in range(8) for x in range(8)))
    return (s + 2) >> 2


# ================================================================ hand-worked answers
def test_nodes_candidate_lists_bits_and_rates():
    assert M.NODES[0] == (0, 0, 32) and M.NODES[4] == (16, 16, 16) and M.NODES[5:9] == [(0, 0, 8), (8, 0, 8), (0, 8, 8), (8, 8, 8)]
    assert [int(M.z_index(x, y)) for x, y in ((0, 0), (4, 0), (0, 4), (4, 4), (8, 0), (16, 0), (0, 16), (28, 28))] == [0, 1, 2, 3, 4, 16, 32, 63]
    # 8.4.2: both neighbours DC -> planar, DC, vertical; both 10 -> 10, 9, 11; both 2 -> 2, 33, 3 (the angular modes wrap round); both 34 -> 34, 33, 3 (8-24: 2 + ((34 - 2 + 1) % 32))
    assert M.cand_mode_list(1, 1) == [0, 1, 26] and M.cand_mode_list(0, 0) == [0, 1, 26]
    assert M.cand_mode_list(10, 10) == [10, 9, 11] and M.cand_mode_list(2, 2) == [2, 33, 3] and M.cand_mode_list(34, 34) == [34, 33, 3]
    # different: the third is planar, unless one of them is planar: then DC, unless the other is DC: then vertical
    assert M.cand_mode_list(10, 26) == [10, 26, 0] and M.cand_mode_list(0, 26) == [0, 26, 1] and M.cand_mode_list(1, 0) == [1, 0, 26]
    assert [M.mode_bits([10, 26, 0], m) for m in (10, 26, 0, 1, 34)] == [2, 3, 3, 6, 6]
    assert [M.level_rate(a) for a in (1, 2, 3, 4, 5, 6, 9, 10, 17, 18)] == [33, 50, 80, 80, 107, 107, 134, 134, 161, 161]
    lv = np.zeros((8, 8), np.int64)
    assert M.coefficient_bits(lv) == 0
    lv[0, 0], lv[1, 3] = -3, 1                         # one sub-block: 143 + 80 + 33, + 30 for the block
    assert M.coefficient_bits(lv) == 286
    lv[7, 7] = 2                                       # a second sub-block: 143 + 50
    assert M.coefficient_bits(lv) == 479
    # SATD: a constant difference of 1 over an 8x8 block leaves one coefficient, 64: (64 + 2) >> 2 = 16; over 4x4: 16, (16 + 1) >> 1 = 8
    assert int(M.satd(np.ones((8, 8)), 8)) == 16 and int(M.satd(np.ones((4, 4)), 4)) == 8
    assert int(M.satd(np.ones((16, 16)), 8)) == 64     # four pieces, each normalised on its own
    one = np.zeros((8, 8), np.int64)
    one[3, 5] = 1                                      # a single sample: 64 coefficients of magnitude 1
    assert int(M.satd(one, 8)) == 16 and satd8_by_hand(one) == 16
    d = np.random.default_rng(1).integers(-200, 200, (8, 8))
    assert int(M.satd(d, 8)) == satd8_by_hand(d)
    assert M.tile_bounds(5, 2) == [0, 2, 5] and M.tile_bounds(3, 2) == [0, 1, 3]


def test_flat_ctu_the_cheapest_bits_win_and_the_tree_is_whole(emu, monkeypatch):
    """Every prediction of a flat picture is exact, so a mode costs its bits.  At the CTU's origin both neighbours are DC (outside the CTU): the list is
    {planar, DC, 26}, planar has the 2 bits.  Along the first row the left node is planar and above is DC: {planar, DC, 26} again.  In the first
    column left is DC and above is planar: {DC, planar, 26}: DC.  Elsewhere: the left node's mode unless it equals the one above (then planar).  That
    gives rows of planar and DC in turn.  Chroma: everything is exact, DM has 1 bit.  Every J is (lambda x 72) >> 4 (2 + 1 + 1.5 bits, nothing coded),
    so whole = J + lambda < lambda + 4 J... = split at both levels."""
    y = np.full((32, 32), 128)                         # one CTU is the whole picture: no reference sample exists, all are 1 << (bd - 1) = 128
    det = []
    p = held(emu, monkeypatch, picture(y), detail=det)[0]
    assert p["chosen"].tolist() == [1] + [0] * 20
    want8 = {(x, yy): (0 if (yy // 8) % 2 == 0 else 1) for x in range(0, 32, 8) for yy in range(0, 32, 8)}
    assert [p["mode"][5 + k] for k in range(16)] == [want8[M.NODES[5 + k][:2]] for k in range(16)]
    assert p["mode"][:5].tolist() == [0, 0, 0, 1, 1] and np.array_equal(p["cmode"], p["mode"])
    lcost, ccost, j, sse, bits = det[0][0]
    assert lcost.tolist() == [2 * LAM_SAD, 3 * LAM_SAD] + [6 * LAM_SAD] * 24 + [3 * LAM_SAD] + [6 * LAM_SAD] * 8
    assert ccost.tolist() == [LAM_SAD] + [3 * LAM_SAD] * 4 and (j, sse, bits) == ((LAM * 72) >> 4, 0, 72)


def test_column_stripes_pick_vertical_and_row_stripes_horizontal(emu, monkeypatch):
    """a picture that depends on x alone is predicted exactly by mode 26 wherever the row above is real (CTUs below the first CTU row): SATD 0, at most 6
    bits, against hundreds of SATD for any other mode.  The same for rows and mode 10, right of the first CTU column.  The 26 / 10 edge filter adds
    (left - corner) >> 1 = 0 there."""
    stripe = np.array([40, 200, 90, 160, 20, 230, 120, 60] * 8)
    col = np.tile(stripe, (64, 1))
    for planes, mode, rows in ((picture(col, col[::2, ::2]), 26, (2, 3)), (picture(col.T, col.T[::2, ::2]), 10, (1, 3))):
        p = held(emu, monkeypatch, planes)
        for ctu in rows:
            assert (p[ctu]["mode"] == mode).all() and (p[ctu]["cmode"] == mode).all(), (mode, ctu, p[ctu])
            assert p[ctu]["chosen"].tolist() == [1] + [0] * 20              # nothing to gain from splitting an exact prediction


def test_diagonal_ramp_picks_a_diagonal_mode_at_a_cost_worked_by_hand(emu, monkeypatch):
    """Y = x + y + 20.  The 8x8 node at (0, 8) of CTU (1, 1) (node 7) has all 33 reference samples: bottom left lies in the CTU to the left, top right in the
    8x8 above it.  Modes 2 and 34 copy along x + y = const, and the [1 2 1] filter they get at 8x8 keeps a linear ramp ((4 t + 2) >> 2 = t): SATD 0.
    The node above it (node 5) has the list {planar, DC, 26}, so 2 and 34 cost 6 bits each and the lower mode, 2, wins.  Node 7's list is then {DC, 2,
    planar}: mode 2 costs 3 lambda, 34 costs 6 lambda.  Planar is NOT exact: p = x + y + 20 + floor((8 - x - y - 2xy) / 16), 3 bits."""
    yy, xx = np.mgrid[0:64, 0:64]
    det = []
    p = held(emu, monkeypatch, picture(xx + yy + 20), detail=det)
    assert p[3]["mode"][5] == 2 and p[3]["mode"][7] == 2
    lcost = det[3][7][0]
    assert lcost[2] == 3 * LAM_SAD and lcost[34] == 6 * LAM_SAD
    y, x = np.mgrid[0:8, 0:8]
    err = -((8 - x - y - 2 * x * y) // 16)                     # source - planar prediction
    assert lcost[0] == (satd8_by_hand(err) << 4) + 3 * LAM_SAD
    assert lcost[0] > lcost[34] and sorted(lcost.tolist())[:2] == [3 * LAM_SAD, 6 * LAM_SAD]


def test_top_right_of_the_fourth_8x8_is_not_available():
    """The 8x8 node at (8, 8) of a CTU: its top-right samples (x 16..23, y 7) lie in the second 16x16, which comes later in z-order, and its bottom-left
    ones (x 0..7, y 16..23) in the third: 16 samples unavailable, all for z-order; top right repeats the last sample above the block.  The node at
    (0, 8) of the same CTU has its top right in the 8x8 above-right, which precedes it: with a CTU to the left nothing is missing."""
    rng = np.random.default_rng(3)
    y = rng.integers(0, 256, (64, 64))
    cov = collections.Counter()
    m = M.IntraPlanModel(picture(y), 8, cov=cov)
    p = m.references(0, 32 + 8, 32 + 8, 8)
    assert cov == {("unavailable", "picture"): 0, ("unavailable", "tile"): 0, ("unavailable", "z-order"): 16}
    assert p[25:].tolist() == [int(y[39, 47])] * 8 and p[17:25].tolist() == y[39, 40:48].tolist() and p[16] == y[39, 39]
    assert p[8:16].tolist() == y[47:39:-1, 39].tolist() and p[:8].tolist() == [int(y[47, 39])] * 8      # bottom left takes the lowest left sample
    cov.clear()
    p = m.references(0, 32, 32 + 8, 8)
    assert not any(cov.values())
    assert p[17:].tolist() == y[39, 32:48].tolist() and p[:16].tolist() == y[55:39:-1, 31].tolist()
    # the same node in the first CTU column: the column to its left is outside the picture, 17 samples
    cov.clear()
    m.references(0, 0, 32 + 8, 8)
    assert cov["unavailable", "picture"] == 17 and cov["unavailable", "z-order"] == 0
    # chroma follows the luma position of its samples: the 4x4 chroma block of the node at (8, 8)
    cov.clear()
    pc = m.references(1, 16 + 4, 16 + 4, 4)
    assert cov["unavailable", "z-order"] == 8 and pc[13:].tolist() == [int(m.p[1][19, 23])] * 4
    # tiles: with a 2 x 2 grid CTU (1, 1) is a tile of its own: nothing around it is available and every sample is 1 << (bd - 1)
    cov.clear()
    mt = M.IntraPlanModel(picture(y), 8, 2, 2, cov)
    assert mt.references(0, 32, 32, 32).tolist() == [128] * 129 and cov["unavailable", "tile"] == 65 and cov["unavailable", "picture"] == 64     # 32 + 1 + 32 in the picture; 32 below and 32 right of it


def test_strong_smoothing_taken_and_missed_by_one(emu, monkeypatch):
    """96x64, CTU (1, 1): the 32x32 node's top line is row 31, x = 31 .. 95.  Flat 100 but the middle sample p[31][-1] = 97 and the last p[63][-1] = 101:
    |100 + 101 - 2 x 97| = 7 < 8: bilinear.  With the last sample 102 the sum is 8: the [1 2 1] filter.  The left line ends below the picture and repeats
    its last sample: |100 + 100 - 200| = 0 on that side."""
    for last, strong in ((101, True), (102, False)):
        y = np.full((64, 96), 100)
        y[31, 63], y[31, 95] = 97, last
        cov = collections.Counter()
        m = M.IntraPlanModel(picture(y), 8, cov=cov)
        p = m.references(0, 32, 32, 32)
        assert (p[64], p[96], p[128]) == (100, 97, last)
        q = R.filter_refs(p, 32, 0, 8, True)
        k = np.arange(63)
        if strong:
            assert q[65:128].tolist() == ((63 - k) * 100 + (k + 1) * last + 32 >> 6).tolist() and q[:65].tolist() == [100] * 65
        else:
            assert q[94:99].tolist() == [100, 99, 99, 99, 100]      # (100 + 200 + 97 + 2) >> 2 = 99, (100 + 194 + 100 + 2) >> 2 = 99
            assert q[127] == 101 and q[128] == 102 and q[:94].tolist() == [100] * 94
        m.luma_satd(32, 32, 32)
        assert (cov["smoothing", "bilinear"] > 0) == strong and (cov["smoothing", "threshold_missed"] > 0) == (not strong)
        det = []
        held(emu, monkeypatch, picture(y), detail=det)
        _, nodes = O.intra_plan(O.Frame(*picture(y)), O.Params(22, 22, 8, LAM_SAD, LAM, 8, 1, 1, 0, 0, 0, 0, 1), detail=True)
        assert nodes[4, 0]["luma_cost"].tolist() == det[4][0][0].tolist()      # the plan of so flat a picture does not move: the costs of the filtered modes do
    # at 10 bit the threshold is 32: 31 passes, 32 does not (8.4.4.2.3: 1 << (BitDepthY - 5))
    for last, strong in ((425, True), (426, False)):
        y = np.full((64, 96), 400)
        y[31, 63], y[31, 95] = 397, last
        cov = collections.Counter()
        M.IntraPlanModel(picture(y, bd=10), 10, cov=cov).luma_satd(32, 32, 32)
        assert (cov["smoothing", "bilinear"] > 0) == strong
        held(emu, monkeypatch, picture(y, bd=10), bd=10)


def test_chroma_34_stands_for_the_luma_mode_and_dm_wins_ties(emu, monkeypatch):
    """Luma: column stripes, mode 26 everywhere below the first CTU row.  Chroma: constant along x + y, which mode 34 copies exactly where the row above
    reaches far enough right (node 0 of CTU (1, 1) in a 96x64 picture: the CTU above right exists).  Among DM (= 26), planar, "26", 10, DC the third
    IS the luma mode and stands for 34: cmode 34 at 3 bits against DM's vertical prediction of a diagonal pattern."""
    stripe = np.array([40, 200, 90, 160, 20, 230, 120, 60] * 12)
    yc, xc = np.mgrid[0:32, 0:48]
    diag = np.array([30, 220, 70, 180, 110, 250, 10, 140] * 10)[xc + yc]
    planes = (np.tile(stripe, (64, 1)), diag, diag.copy())
    det = []
    p = held(emu, monkeypatch, planes, detail=det)
    assert p[4]["mode"][0] == 26 and p[4]["cmode"][0] == 34
    ccost = det[4][0][1]
    assert ccost[2] == 3 * LAM_SAD and ccost[0] > ccost[2] and int(np.argmin(ccost)) == 2
    assert held(emu, monkeypatch, planes, chroma_modes=0)[4]["cmode"][0] == 26        # chroma_modes = 0: always DM
    # a tie: DM costs 16 SATD_DM + lambda, another candidate 16 SATD + 3 lambda: equal when lambda = 8 (SATD_DM - SATD).  The 8x8 node at (8, 8) of CTU 3
    # of the 64x64 test picture (node 8; luma: planar) at lambda 8: DM and horizontal both cost 3000: DM keeps it.  At lambda 7: 2999 against 2997: it loses
    src = util.planes3(util.plan_case_source("synth", 64, 64, 8))
    det = []
    p = held(emu, monkeypatch, src, lam_sad=8, detail=det)
    ccost = det[3][8][1]
    assert ccost.tolist() == [3000, 5304, 6632, 3000, 4600] and (p[3]["mode"][8], p[3]["cmode"][8]) == (0, 0)
    det = []
    p = held(emu, monkeypatch, src, lam_sad=7, detail=det)
    assert det[3][8][1].tolist() == [2999, 5301, 6629, 2997, 4597] and (p[3]["mode"][8], p[3]["cmode"][8]) == (0, 10)


def test_tree_with_whole_equal_to_split(emu, monkeypatch):
    """lambda = 0 on a flat CTU: every J is 0, whole = split = 0 at both levels, and the whole node keeps the tie: one 32x32 leaf.  (With any lambda > 0 a
    node that codes nothing is cheaper whole, so an exact tie needs lambda = 0: J is then 16 SSE alone.)"""
    y = np.full((32, 32), 128)
    p = held(emu, monkeypatch, picture(y), lam=0)[0]
    assert p["chosen"].tolist() == [1] + [0] * 20
    # the same on column stripes, where every node of CTU 3 is predicted exactly (SSE 0, nothing coded) and lambda = 0 leaves 0 against 0 at both levels
    col = np.tile(np.array([40, 200, 90, 160, 20, 230, 120, 60] * 8), (64, 1))
    p = held(emu, monkeypatch, picture(col, col[::2, ::2]), lam=0)
    assert p[3]["chosen"].tolist() == [1] + [0] * 20 and p[2]["chosen"].tolist() == [1] + [0] * 20


# ================================================================ model == oracle == stepped kernel on the cases of tests/util.py
@pytest.mark.parametrize("c", PLAN_CASES, ids=[c.id for c in PLAN_CASES])
def test_plan_model_oracle_and_stepped_kernel_agree(emu, monkeypatch, c):
    want, prm, cp = plan_case_want(c)
    src = plan_case_source(c.content, c.w, c.h, c.bd)
    if c.content == "rails":
        assert util.reaches_both_ends(src, c.bd, 0.01)
    orc, nodes = O.intra_plan(src, prm, detail=True)
    if orc.tobytes() != want.tobytes():
        pytest.fail("oracle != model: " + plan_diff(orc, want) + explain(c, nodes, orc, want))
    for order, fill in LANE_ORDERS:
        monkeypatch.setenv("EMU_ORDER", order)
        if fill:
            monkeypatch.setenv("EMU_SHARED_FILL", fill)
        got = emu.intra_plan(src, cp)
        assert got.tobytes() == want.tobytes(), f"stepped kernel (lane order {order}) != model: " + plan_diff(got, want)


def explain(c, nodes, orc, want):
    """where the arrays differ, the oracle's table against the model's says which term"""
    det = []
    _, _, cp = plan_case_want(c)
    util.plan_model(c.content, c.w, c.h, c.bd, c.tiles).plan(cp.qp, cp.qp_c, cp.lambda_sad_q4, cp.lambda_q4, c.chroma_modes, det)
    for ctu, info in enumerate(det):
        for nd, (lcost, ccost, j, sse, bits) in info.items():
            o = nodes[ctu, nd]
            if not np.array_equal(o["luma_cost"], lcost):
                k = np.nonzero(o["luma_cost"] != lcost)[0]
                return f"; CTU {ctu} node {nd}: luma cost of modes {k.tolist()}: oracle {o['luma_cost'][k].tolist()}, model {lcost[k].tolist()}"
            if ccost is not None and not np.array_equal(o["chroma_cost"], ccost):
                return f"; CTU {ctu} node {nd}: chroma costs oracle {o['chroma_cost'].tolist()}, model {ccost.tolist()}"
            if (int(o["sse"]), int(o["bits_q4"]), int(o["j"])) != (sse, bits, j):
                return f"; CTU {ctu} node {nd}: SSE / bits / J oracle {(int(o['sse']), int(o['bits_q4']), int(o['j']))}, model {(sse, bits, j)}"
    return "; every cost agrees: the difference is in a tie or in the tree"


def test_the_model_alone_reaches_every_rule():
    for c in PLAN_CASES:
        plan_case_want(c)
    cov = PLAN_COVERAGE
    want = [("luma", m) for m in range(35)] + [("chroma", k) for k in ("DM", "planar", "vertical", "horizontal", "DC", "34 for the luma mode")]
    want += [("cand_from", k) for k in ("equal, non-angular", "equal, angular", "different")]
    want += [("smoothing", "bilinear"), ("smoothing", "threshold_missed"), ("leaf", 32), ("leaf", 16), ("leaf", 8), "invalid node"]
    want += [("unavailable", k) for k in ("picture", "tile", "z-order")]
    missing = [k for k in want if not cov[k]]
    print({str(k): cov[k] for k in want})
    assert not missing, missing


# ================================================================ the code stage carries the plan
@pytest.mark.parametrize("nxn", [0, 1])
@pytest.mark.parametrize("name", ["136x72-8bit-qp22-cm1", "72x104-10bit-qp32-cm1", "64x64-8bit-qp42-cm0", "tiles2x2-136x72-10bit-qp27"])
def test_cu_records_carry_the_plan(emu, name, nxn):
    c = next(k for k in PLAN_CASES if k.id == name)
    want, prm0, cp0 = plan_case_want(c)
    prm, cp = type(prm0).from_buffer_copy(prm0), type(cp0).from_buffer_copy(cp0)
    prm.intra_nxn = cp.intra_nxn = nxn
    src = plan_case_source(c.content, c.w, c.h, c.bd)
    for a in (O.analyze_intra(src, prm), emu.intra(src, cp)):
        check_records_carry_the_plan(want, a.cu, c.w, c.h, nxn)
        if nxn and name == "136x72-8bit-qp22-cm1":
            assert (a.cu["flags"] & 16).any(), "no NxN CU: the case does not test what it is for"
