"""GPU: the intra code stage, the NxN trial (mihevc_k_intra_frame) and the intra second pass of P pictures (mihevc_k_inter_frame with intra_in_p) of the
real gfx950 kernels held to tests/hevc_intra_code.py, the brute-force numpy model written from DESIGN.md §6, WITHOUT the oracle in between: CU records,
levels, pre-deblock reconstruction and rate estimate, exactly.  The hand-made pictures of the CPU file, then 64x64 and 136x72 at 8 and 10 bit, QP 22 and
42, NxN on, the 2 x 2 tile grids, the pictures with J_nxn == J_2Nx2N, and four P pictures (isolated and paired candidates, a tile grid, a candidate that
stays inter).  tests/test_intra_code_independent.py is the CPU twin (oracle and stepped kernel sources, every case, coverage and binding counts).  The
model's results are computed once per case (tests/util.py keeps them)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import hevc_intra_code as M
from tests import hevc_intra_plan as P
from tests import util
from tests.test_intra_code_independent import checker_pair, flat_step_pair, quadrant_picture
from tests.util import (GPU_CODE_CASES, GPU_P_CODE_CASES, P_CODE_CASES, code_case_params, code_case_want, inter_diff, p_code_case_params, p_code_case_pictures,
                        p_code_case_want, plan_case_source)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from hevc_amd import _lib
    lib = _lib.load()
    assert lib.mihevc_device_count() >= 1
    return util.StageApi(lib, "mihevc_k_", device=0)


def test_the_device_cases_are_the_ones_asked_for():
    plain = {(c.plan.w, c.plan.h, c.plan.bd, c.plan.qp) for c in GPU_CODE_CASES if c.plan.tiles == (1, 1) and c.plan.lam is None}
    assert plain == {(w, h, bd, qp) for (w, h) in ((64, 64), (136, 72)) for bd in (8, 10) for qp in (22, 42)}
    assert all(c.nxn == 1 for c in GPU_CODE_CASES) and any(c.plan.tiles == (2, 2) for c in GPU_CODE_CASES) and any(c.plan.lam is not None for c in GPU_CODE_CASES)
    assert len(GPU_P_CODE_CASES) == 4 and {c.bd for c in GPU_P_CODE_CASES} == {8, 10} and any(c.tiles == (2, 2) for c in GPU_P_CODE_CASES)


def device_i(api, planes, bd=8, qp=22, nxn=1, tiles=(1, 1), **lambdas):
    """a hand-made I picture on the device against the model (the model's own plan)"""
    _, cp = util.params_pair(qp, bd, 8, intra_nxn=nxn, chroma_modes=1, tile_cols=tiles[0], tile_rows=tiles[1], **lambdas)
    plan = P.plan_picture(planes, bd, cp.qp, cp.qp_c, cp.lambda_sad_q4, cp.lambda_q4, tiles[0], tiles[1], 1)
    want = M.code_picture(planes, plan, util.model_params(cp))
    d = inter_diff(want, api.intra(O.Frame(*planes), cp))
    assert not d, "mihevc_k_intra_frame != model: " + d
    return want


def test_device_pins_of_the_code_stage(api):
    """the hand-worked pictures of the CPU file: flat (nothing coded, 128 per CU), column stripes with and without a tile edge left of CTU (1, 1), flat luma
    under textured chroma (no trial)"""
    v = np.full((64, 64), 128)
    assert device_i(api, (v, v[::2, ::2], v[::2, ::2])).est == 4 * 128
    stripes = util.planes3(plan_case_source("stripes", 64, 64, 8))
    assert device_i(api, stripes).cus[32, 32]["cand"] == [26, 1, 0] and device_i(api, stripes, tiles=(2, 1)).cus[32, 32]["cand"] == [0, 1, 26]
    rng = np.random.default_rng(5)
    r = device_i(api, (np.full((24, 24), 128), rng.integers(40, 220, (12, 12)), rng.integers(40, 220, (12, 12))))
    assert r.cov["nxn", "not tried, chroma has a level"] >= 3 and not (r.cu["flags"] & 16).any()


def test_device_pins_of_the_nxn_trial(api):
    """four directions in one CU: NxN wins with four different modes; at lambda_q4 = 0 and QP 0 two CUs cost the same both ways and stay 2Nx2N"""
    r = device_i(api, quadrant_picture(24, 24))
    assert r.cus[16, 0]["nxn"]["kept"] and len(set(r.cus[16, 0]["nxn"]["modes"])) == 4
    r = device_i(api, quadrant_picture(24, 24), qp=0, lambda_q4=0)
    assert [r.cus[xy]["nxn"]["j_nxn"] - r.cus[xy]["nxn"]["j_2nx2n"] for xy in ((16, 8), (16, 16))] == [0, 0] and not r.cus[16, 8]["nxn"]["kept"]


def test_device_unrelated_picture_converts_two_ctus(api):
    c = next(k for k in P_CODE_CASES if k.content == "unrelated")
    want = p_code_case_want(c)
    cur, ref = p_code_case_pictures(c)
    got = api.inter(cur, ref, p_code_case_params(c)[1])
    d = inter_diff(want, got)
    assert not d, "mihevc_k_inter_frame != model: " + d
    assert ((got.cu["flags"] & 1) == 0).sum() == 32 and ((got.cu["flags"] & 1) == 0)[:4, :8].all()


@pytest.mark.parametrize("mean,amp,candidate", [(128, 40, False), (129, 15, True), (128, 16, False)])
def test_device_candidate_tests_at_their_boundaries(api, mean, amp, candidate):
    """the checkerboards of the CPU file: cost == act << 4 exactly (no candidate), cost == 4 per sample exactly (a candidate, replaced), both at once"""
    _, cp = util.params_pair(22, 8, 8, intra_in_p=1, chroma_modes=1, intra_nxn=1, lambda_sad_q4=0)
    cur, ref = checker_pair(mean, amp)
    want = M.second_pass(util.planes3(cur), util.planes3(ref), util.model_params(cp))
    assert want.ctus[0]["candidate"] == candidate and bool(want.ctus[0].get("replaced")) == candidate
    got = api.inter(cur, ref, cp)
    d = inter_diff(want, got)
    assert not d, "mihevc_k_inter_frame != model: " + d
    assert bool((got.cu["flags"] & 1).all()) == (not candidate)


@pytest.mark.parametrize("qp", [22, 32])
def test_device_intra_at_equal_cost_stays_inter(api, qp):
    """flat 144 against flat 128 at both lambdas 0: both CTUs are tried, J_ctu == jinter == 0, and the inter version stays"""
    _, cp = util.params_pair(qp, 8, 8, intra_in_p=1, chroma_modes=1, intra_nxn=1, lambda_sad_q4=0, lambda_q4=0)
    cur, ref = flat_step_pair()
    want = M.second_pass(util.planes3(cur), util.planes3(ref), util.model_params(cp))
    assert all(t["round"] >= 0 and t["j_ctu"] == t["jinter"] == 0 and not t["replaced"] for t in want.ctus.values())
    got = api.inter(cur, ref, cp)
    d = inter_diff(want, got)
    assert not d, "mihevc_k_inter_frame != model: " + d
    assert (got.cu["flags"] & 1).all() and got.est == want.inter.est


@pytest.mark.parametrize("c", GPU_CODE_CASES, ids=[c.id for c in GPU_CODE_CASES])
def test_device_i_picture_equals_the_model(api, c):
    want = code_case_want(c)
    d = inter_diff(want, api.intra(plan_case_source(c.plan.content, c.plan.w, c.plan.h, c.plan.bd), code_case_params(c)[1]))
    assert not d, "mihevc_k_intra_frame != model: " + d


@pytest.mark.parametrize("c", GPU_P_CODE_CASES, ids=[c.id for c in GPU_P_CODE_CASES])
def test_device_p_picture_equals_the_model(api, c):
    want = p_code_case_want(c)
    cur, ref = p_code_case_pictures(c)
    d = inter_diff(want, api.inter(cur, ref, p_code_case_params(c)[1]))
    assert not d, "mihevc_k_inter_frame != model: " + d
    assert any(t.get("replaced") for t in want.ctus.values()), "no CTU replaced: the case does not test what it is for"
