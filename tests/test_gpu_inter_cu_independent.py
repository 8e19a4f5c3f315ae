"""GPU: what the real gfx950 kernels `k_inter_ctu` / `k_inter_ctu_b` decide (through mihevc_k_inter_frame / mihevc_k_b_frame) held to tests/hevc_inter_cu.py,
the brute-force numpy model written from DESIGN.md §6, WITHOUT the oracle in between: every case of util.INTER_CASES (64x64 / 136x72 / 72x104, 8 and 10 bit,
me_range 8 / 15, QP 22 / 32 / 42, rdo_zero 0 / 1, explicit centres, the pre-search, slices, lambda_sad_q4 = 0, B pictures, the residual-rich pictures with
rdo_cg 0 / 2 / 5 / 8: records, levels, reconstruction and estimate of every case) and the hand-worked pictures (the group drop at its equality among them) of
tests/test_inter_cu_independent.py, its CPU twin (oracle, stepped kernel sources, the coverage count).  The model's answer is computed once per case."""
import numpy as np
import pytest

from tests import util
from tests.util import INTER_CASES, INTER_PINS, inter_case_want, inter_diff, run_inter_case

pytestmark = pytest.mark.gpu

CASES = list(INTER_PINS.values()) + INTER_CASES


@pytest.fixture(scope="module")
def api():
    from hevc_amd import _lib
    lib = _lib.load()
    assert lib.mihevc_device_count() >= 1
    return util.StageApi(lib, "mihevc_k_", device=0)


def test_the_device_cases_include_the_pins_and_the_ties():
    ids = {c.id for c in CASES}
    assert ids >= set(INTER_PINS) and len(ids) == len(CASES)
    assert sum(1 for c in CASES if c.lam is not None and c.lam[0] == 0) >= 9 and any(c.content.startswith("b-same") and c.lam for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_device_analysis_equals_the_model(api, c):
    want, me, _ = inter_case_want(c)
    got = run_inter_case(api, c)
    for l, m in enumerate(me):
        t = got.me if len(me) == 1 else got.me[l]
        assert np.array_equal(t, m), f"integer table, list {l}: device != model: " + util.first_diff(t, m)
    d = inter_diff(want, got)
    assert not d, "device != model: " + d
