"""GPU (-m gpu): the device's search centres, integer-search dump and SAO parameters against tests/hevc_analysis.py, the numpy model written from
DESIGN.md §6 — exactly, on the cases of tests/util.py (those of tests/test_analysis_independent.py), and without the oracle: the pictures the SAO cases judge are the device's
own (intra / inter analysis and deblocking through the stage entry points)."""
import numpy as np
import pytest

from tests import hevc_analysis as A
from tests import util
from tests.util import (ALL_SAO_KINDS, B_CASE, SAO_CASES, SEARCH_CASES, audit_search, b_case_centres, b_case_pictures, case_centres, case_pictures, check_planted,
                        first_diff, params_pair, planes3, planted_sao_input, sao_case_sources, sao_diff, sao_kinds)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from hevc_amd import _lib
    lib = _lib.load()
    assert lib.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return util.StageApi(lib, "mihevc_k_", device=0)


@pytest.mark.parametrize("c", SEARCH_CASES, ids=[c.id for c in SEARCH_CASES])
def test_integer_search_on_the_device_equals_the_model(api, c):
    _, cp = params_pair(27, c.bd, c.R, pre_search=c.pre_search)
    cur, ref = case_pictures(c)
    cen = case_centres(c)
    want = audit_search(c, cur, ref, cp.lambda_sad_q4, cen)
    check_planted(c, want, cp.lambda_sad_q4)
    got = api.inter(cur, ref, cp, centers=cen)
    assert np.array_equal(got.me, want), first_diff(got.me, want)


def test_b_picture_both_lists_on_the_device(api):
    c = B_CASE
    _, cp = params_pair(27, c.bd, c.R)
    cur, ref0, ref1 = b_case_pictures()
    cen1 = b_case_centres()
    want = (A.integer_search(cur.y, ref0.y, c.bd, c.R, cp.lambda_sad_q4), A.integer_search(cur.y, ref1.y, c.bd, c.R, cp.lambda_sad_q4, cen1))
    got = api.b(cur, ref0, ref1, cp, None, cen1)
    for l in range(2):
        assert np.array_equal(got.me[l], want[l]), f"list {l}: " + first_diff(got.me[l], want[l])


_sao_seen = {}


def device_sao_run(api, c):
    """the SAO parameters of k_sao and of the fused loop filter for the case's pictures, each checked against the model; returns the kinds reached"""
    if c.id in _sao_seen:
        return _sao_seen[c.id]
    _, cp = params_pair(c.qp, c.bd, 8)
    kinds = set()
    if c.content == "planted":
        src, d = planted_sao_input(c)
        want = A.sao_parameters(planes3(src), planes3(d), c.bd, cp.lambda_q4)
        got = api.sao(src, d, cp)[1]
        assert got.tobytes() == want.tobytes(), "k_sao != model: " + sao_diff(got, want)
        kinds |= sao_kinds(got)
    else:
        ref = None
        for i, src in enumerate(sao_case_sources(c)):
            a = api.intra(src, cp) if i == 0 else api.inter(src, ref, cp)
            d = api.deblock(a.rec, a.cu, c.bd)
            want = A.sao_parameters(planes3(src), planes3(d), c.bd, cp.lambda_q4)
            ref, got = api.sao(src, d, cp)
            assert got.tobytes() == want.tobytes(), f"picture {i}: k_sao != model: " + sao_diff(got, want)
            fused = api.loop_filter(src, a.rec, a.cu, cp)[1]
            assert fused.tobytes() == want.tobytes(), f"picture {i}: fused loop filter != model: " + sao_diff(fused, want)
            kinds |= sao_kinds(got)
    _sao_seen[c.id] = kinds
    return kinds


@pytest.mark.parametrize("c", SAO_CASES, ids=[c.id for c in SAO_CASES])
def test_sao_parameters_on_the_device_equal_the_model(api, c):
    device_sao_run(api, c)


def test_sao_cases_reach_every_type_and_class_on_the_device(api):
    seen = set()
    for c in SAO_CASES:
        seen |= device_sao_run(api, c)
    assert seen == ALL_SAO_KINDS, sorted(ALL_SAO_KINDS - seen)
