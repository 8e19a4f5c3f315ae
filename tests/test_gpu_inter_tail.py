"""GPU (-m gpu): the cases of tests/test_inter_tail_cpu.py through the device entries (mihevc_k_*) against the oracle, and one short session with sign data
hiding against the fixture the commit before the block-wise tail stages wrote (tests/golden/streams_inter_tail.json).  The device entries take sign data
hiding from a session's configuration only, so the stage cases run without it and the session carries it."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O
from tests import util
from tests import test_inter_tail_cpu as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


class DeviceApi:
    """the device entries behind the calls the CPU file makes: they take a mihevc_cost_params, the cases carry the oracle's Params (the same fields)"""

    def __init__(self, lib):
        self.api = util.StageApi(lib, "mihevc_k_", device=0)

    @staticmethod
    def cost(prm):
        from hevc_amd import _lib
        cp = _lib.CostParams()
        assert [n for n, _ in _lib.CostParams._fields_] == [n for n, _ in O.Params._fields_]
        for n, _ in O.Params._fields_:
            setattr(cp, n, getattr(prm, n))
        return cp

    def intra(self, src, prm):
        return self.api.intra(src, self.cost(prm))

    def inter(self, src, ref, prm, centers=None):
        return self.api.inter(src, ref, self.cost(prm), centers)

    def b(self, src, ref0, ref1, prm, centers0=None, centers1=None):
        return self.api.b(src, ref0, ref1, self.cost(prm), centers0, centers1)


@pytest.fixture(scope="module")
def api(lib):
    return DeviceApi(lib)


@pytest.mark.parametrize("shape,qp,rz,cg", T.CASES, ids=["-".join(map(str, c)) for c in T.CASES])
def test_device_p_pictures(api, shape, qp, rz, cg):
    T.check_p({0: api}, shape, qp, rz, cg, 0)


def test_device_intra_second_pass_sums(api):
    T.test_intra_second_pass_sums({0: api})


def test_device_b_picture(api):
    T.test_b_picture({0: api})


def test_device_idr_picture_with_tiles_nxn_and_chroma_modes(api):
    T.test_idr_picture_with_tiles_nxn_and_chroma_modes({0: api})


def test_session_produces_the_golden_pictures(lib):
    """12 pictures of 136x72, keyint 6, two GOP lanes, sign_hide 1: the bytes and reconstructions of the fixture"""
    from hevc_amd.encoder import Encoder
    golden = Path(__file__).parent / "golden"
    spec = importlib.util.spec_from_file_location("make_inter_tail_goldens", golden / "make_inter_tail_goldens.py")
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    want = json.loads((golden / "streams_inter_tail.json").read_text())[G.NAME]
    S = G.helper()
    cfg = S.config(G.NAME)
    assert (cfg.width, cfg.height, cfg.keyint, cfg.gops_in_flight, cfg.sign_hide) == (136, 72, 6, 2, 1)
    n = G.CASE[3]
    with Encoder(cfg, device=0, keep_recon=True) as enc:
        for f in S.frames(G.NAME):
            enc.send(*util.planes(f, cfg.bit_depth))
        enc.flush()
        packets = [d for d, _pts, _key in enc.packets()]
        headers = enc.headers()
        recs = [O.Frame(*enc.recon(i)) for i in range(n)]
    assert len(packets) == n == 12 and packets[0].startswith(headers)
    packets[0] = packets[0][len(headers):]
    assert [len(p) for p in packets] == want["bytes"]
    assert [S.sha(p) for p in packets] == want["pictures"]
    assert [S.frame_hash(r) for r in recs] == want["recon"]
