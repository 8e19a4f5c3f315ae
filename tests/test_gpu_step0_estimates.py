"""GPU (-m gpu): step 0 of a session's first chunk under rate control decides what it decided before its estimates travelled differently.

idr_step and rho_trial (hevc_amd/csrc/session.cpp) read every lane's rate estimate back from the device: the copies are queued behind the launches that
produce the words and the host waits once, where it used to synchronise and then make one blocking copy per lane.  The word read is the same word, so every
QP the rate controller derives from it, and with it every coded size, must be the same.  tests/golden/step0_estimates.json was recorded by the commit before
that change (tests/golden/make_step0_goldens.py, which also holds the cases and their inputs): 256x128, keyint 4, CRF 20 under a cap,
 - flat content whose first IDR analysis already sits at the QP the cap asks for: one analysis,
 - white noise under a cap of a tenth of what it takes: the trial, then every lane analysed a second time,
 - the same with a single lane.
The number of IDR analyses (mihevc_stats.stage_launches[0] with profile_stages 1) is part of the fixture and is asserted outright: a case that stopped
taking its path would not pass by doing less."""
import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"


def _maker():
    spec = importlib.util.spec_from_file_location("make_step0_goldens", GOLDEN / "make_step0_goldens.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


M = _maker()
WANT = json.loads((GOLDEN / "step0_estimates.json").read_text())


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


def test_the_fixture_covers_both_paths():
    assert set(WANT) == set(M.CASES)
    assert WANT["flat_no_redo"]["idr_analyses"] == 1 and WANT["noise_redo"]["idr_analyses"] == 2 and WANT["single_lane"]["idr_analyses"] == 2
    assert len(WANT["single_lane"]["qp"]) == 4 and len(WANT["noise_redo"]["qp"]) == 16
    for name, w in WANT.items():
        assert [i for i, t in enumerate(w["type"]) if t == 2] == list(range(0, len(w["type"]), M.KEYINT)), name


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_first_chunk_decides_as_recorded(lib, name):
    got, want = M.compute(name), WANT[name]
    assert got["idr_analyses"] == M.CASES[name][6] == want["idr_analyses"], "the case no longer takes its path through step 0"
    assert got["qp"] == want["qp"], "a QP of the first chunk moved"
    assert got["type"] == want["type"] and got["pts"] == want["pts"]
    assert got["bits"] == want["bits"] and got["packet_bytes"] == want["packet_bytes"], "a coded size of the first chunk moved"
