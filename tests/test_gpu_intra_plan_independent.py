"""GPU: the intra plan of the real gfx950 kernel (mihevc_k_intra_plan) held to tests/hevc_intra_plan.py, the brute-force numpy model written from
DESIGN.md §6, WITHOUT the oracle in between: 64x64 and 136x72 at 8 and 10 bit, QP 22 and 42, chroma modes on, the 2 x 2 tile grids, and the hand-made
pictures whose answer hangs on an exact tie or a threshold (lambda_q4 = 0: whole == split; the DM tie; the strong-smoothing line).  Then the code
stage (mihevc_k_intra_frame) must carry that plan: every CU record has its leaf's size and modes.  tests/test_intra_plan_independent.py is the CPU twin
(oracle and stepped kernel sources, every case, the coverage count)."""
import numpy as np
import pytest

from tests import util
from tests.util import GPU_PLAN_CASES, check_records_carry_the_plan, plan_case_source, plan_case_want, plan_diff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from hevc_amd import _lib
    lib = _lib.load()
    assert lib.mihevc_device_count() >= 1
    return util.StageApi(lib, "mihevc_k_", device=0)


def test_the_device_cases_are_the_ones_asked_for():
    plain = {(c.w, c.h, c.bd, c.qp) for c in GPU_PLAN_CASES if c.tiles == (1, 1) and c.content == "synth" and c.lam is None}
    assert plain == {(w, h, bd, qp) for (w, h) in ((64, 64), (136, 72)) for bd in (8, 10) for qp in (22, 42)}
    assert all(c.chroma_modes == 1 for c in GPU_PLAN_CASES) and any(c.tiles == (2, 2) for c in GPU_PLAN_CASES)
    # and the exact ties and thresholds of the hand-worked CPU cases: lambda_q4 = 0 (whole == split), the DM tie and one less, the smoothing line by one
    assert {c.lam for c in GPU_PLAN_CASES} >= {(38, 0), (8, 92), (7, 92)} and {c.content for c in GPU_PLAN_CASES} >= {"flat", "stripes", "line7", "line8", "line31", "line32"}


@pytest.mark.parametrize("c", GPU_PLAN_CASES, ids=[c.id for c in GPU_PLAN_CASES])
def test_device_plan_equals_the_model(api, c):
    want, _, cp = plan_case_want(c)
    got = api.intra_plan(plan_case_source(c.content, c.w, c.h, c.bd), cp)
    assert got.tobytes() == want.tobytes(), "mihevc_k_intra_plan != model: " + plan_diff(got, want)


@pytest.mark.parametrize("nxn", [0, 1])
@pytest.mark.parametrize("name", ["136x72-8bit-qp22-cm1", "64x64-10bit-qp42-cm1", "tiles2x2-136x72-10bit-qp27"])
def test_device_cu_records_carry_the_plan(api, name, nxn):
    c = next(k for k in GPU_PLAN_CASES if k.id == name)
    want, _, cp0 = plan_case_want(c)
    cp = type(cp0).from_buffer_copy(cp0)
    cp.intra_nxn = nxn
    a = api.intra(plan_case_source(c.content, c.w, c.h, c.bd), cp)
    check_records_carry_the_plan(want, a.cu, c.w, c.h, nxn)
    if nxn:
        assert name != "136x72-8bit-qp22-cm1" or (a.cu["flags"] & 16).any(), "no NxN CU: the case does not test what it is for"


def test_bad_arguments_are_refused_before_any_launch(api):
    import ctypes as C
    from hevc_amd import _lib
    c = GPU_PLAN_CASES[0]
    _, _, cp0 = plan_case_want(c)
    cp = type(cp0).from_buffer_copy(cp0)
    cp.tile_cols = 3                                   # 64x64 has two CTU columns
    s = util.planes(plan_case_source(c.content, c.w, c.h, c.bd), c.bd)
    plan = np.zeros(util.n_ctus(c.w, c.h), util.O.INTRA_PLAN_DTYPE)
    f = api.lib.mihevc_k_intra_plan
    assert f(0, util.ptr(s[0]), util.ptr(s[1]), util.ptr(s[2]), c.w, c.h, C.byref(cp), util.ptr(plan)) == _lib.EINVAL
    assert f(0, util.ptr(s[0]), util.ptr(s[1]), util.ptr(s[2]), c.w, c.h, C.byref(cp0), None) == _lib.EINVAL
    assert f(0, util.ptr(s[0]), util.ptr(s[1]), util.ptr(s[2]), c.w + 4, c.h, C.byref(cp0), util.ptr(plan)) == _lib.EINVAL
