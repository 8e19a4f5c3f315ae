"""GPU (-m gpu): both forms of k_me_search -- the one compiled for me_range 15 (compile-time window stride, the quad-SAD operands read as 8-byte pairs)
and the one that takes the range from its arguments -- and the P stage behind them (k_inter_ctu: unbiased filtered rows, row base split once per
candidate), through the stage entry mihevc_k_inter_frame as tests/test_gpu_parity.py drives it, against the oracle (orc_analyze_inter_frame), bit for
bit: vectors and costs of all 21 nodes of every CTU, then records, levels, reconstruction and rate estimate.  96 x 80 (partial CTUs at the bottom
edge; 88 x 72 adds a partial column at the right edge), 8 and 10 bit, with and without search centres.  The oracle's analysis of a case is computed
once and shared by the tests that read it."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import util

pytestmark = pytest.mark.gpu

SIZES = [(96, 80), (88, 72)]
CASES = [pytest.param(w, h, bd, rng, cen, id=f"{w}x{h}-{bd}bit-range{rng}-{'centres' if cen else 'origin'}")
         for (w, h) in SIZES for bd in (8, 10) for rng in (15, 7) for cen in (False, True) if (w, h) == SIZES[0] or (rng == 15 and cen)]


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


@pytest.fixture(scope="module")
def api(lib):
    return util.StageApi(lib, "mihevc_k_", device=0)


_runs = {}


def run(api, w, h, bd, rng, cen):
    """(oracle analysis, device analysis) of one P picture, computed once per case"""
    key = (w, h, bd, rng, cen)
    if key not in _runs:
        from hevc_amd import _lib
        cp = _lib.cost_params(26, bd, rng)
        prm = O.Params(cp.qp, cp.qp_c, cp.bit_depth, cp.lambda_sad_q4, cp.lambda_q4, cp.me_range)
        assert cp.me_range == rng
        ref = util.synth_frame(h, w, 5, bit_depth=bd)
        src = util.synth_frame(h, w, 5, shift=(11, -6), bit_depth=bd)       # inside +-15 of the origin, outside +-7 of it, inside +-7 of the centres
        centres = None
        if cen:
            centres = np.zeros((util.n_ctus(w, h), 2), np.int16)
            centres[:, 0], centres[:, 1] = 10, -5
            centres[1::2] = (-3, 4)                                         # not every CTU alike
        want = O.analyze_inter(src, ref, prm, centers=centres, dump_me=True)
        _runs[key] = (want, api.inter(src, ref, cp, centers=centres))
    return _runs[key]


@pytest.mark.parametrize("w,h,bd,rng,cen", CASES)
def test_integer_search_equals_oracle_in_both_range_forms(api, w, h, bd, rng, cen):
    want, got = run(api, w, h, bd, rng, cen)
    assert want.me.shape == got.me.shape == (util.n_ctus(w, h), 21, 3)
    assert np.array_equal(want.me[:, :, :2], got.me[:, :, :2]), "vectors differ at (ctu, node) " + str(np.argwhere((want.me != got.me).any(axis=2))[:4].tolist())
    assert np.array_equal(want.me[:, :, 2], got.me[:, :, 2]), "costs differ at (ctu, node) " + str(np.argwhere(want.me[:, :, 2] != got.me[:, :, 2])[:4].tolist())
    assert (want.me[:, :, 2] >= 0).any() and (want.me[:, :, 2] < 0).any()       # nodes inside the picture, and nodes of partial CTUs outside it


@pytest.mark.parametrize("w,h,bd,rng,cen", CASES)
def test_p_stage_equals_oracle_in_both_range_forms(api, w, h, bd, rng, cen):
    want, got = run(api, w, h, bd, rng, cen)
    assert util.same_analysis(want, got), util.describe_diff(want, got)
    assert (want.cu["flags"] & 1).any()                                         # inter CUs: the fractional search and motion compensation ran
