"""GPU (-m gpu): sign data hiding (mihevc_config.sign_hide) on an MI355X.  K3 with sign hiding (mihevc_k_transform_sdh, the DST-VII 4x4 path included)
against the numpy rule of tests/test_sign_hiding_cpu.py; sessions at the golden SDH cases produce the fixture's bytes; full-size sessions with the
default session features decode with the repository's decoder (its own sign inference) to the session's reconstruction, bit for bit."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import util
from tests.test_gpu_configs import clip_frames, operating_point
from tests.test_sign_hiding_cpu import S, WANT, k3_grid, k3_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


def test_k_transform_sdh_equals_the_numpy_rule(lib):
    def call(res, lvl, rec, count, log2n, qp, bd, intra, dst, scan):
        assert lib.mihevc_k_transform_sdh(0, util.ptr(res), util.ptr(lvl), util.ptr(rec), count, log2n, qp, bd, intra, int(dst), scan, 1) == 0
    changed = 0
    for i, (log2n, scan, bd, qp, kind) in enumerate(k3_grid()):
        changed += k3_run(call, log2n, scan, bd, qp, kind, intra=i % 2)
        if log2n == 2:
            changed += k3_run(call, log2n, scan, bd, qp, kind, intra=1, dst=True)          # the NxN trial's DST-VII luma blocks
    assert changed > 500
    # switched off it is mihevc_k_transform
    res = np.random.default_rng(1).integers(-255, 256, (16, 8, 8)).astype(np.int16)
    a, b = [np.zeros_like(res) for _ in range(2)], [np.zeros_like(res) for _ in range(2)]
    assert lib.mihevc_k_transform(0, util.ptr(res), util.ptr(a[0]), util.ptr(a[1]), 16, 3, 22, 8, 1, 0) == 0
    assert lib.mihevc_k_transform_sdh(0, util.ptr(res), util.ptr(b[0]), util.ptr(b[1]), 16, 3, 22, 8, 1, 0, 0, 0) == 0
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_session_produces_the_golden_sdh_pictures(lib, name):
    from hevc_amd.encoder import Encoder
    cfg = S.config(name)
    bd, n = cfg.bit_depth, S.CASES[name][3]
    with Encoder(cfg, device=0, keep_recon=True) as enc:
        for f in S.frames(name):
            enc.send(*util.planes(f, bd))
        enc.flush()
        packets = [d for d, _pts, _key in enc.packets()]
        headers = enc.headers()
        recs = [O.Frame(*enc.recon(i)) for i in range(n)]
    assert packets[0].startswith(headers)
    packets[0] = packets[0][len(headers):]
    assert [len(p) for p in packets] == WANT[name]["bytes"]
    assert [S.sha(p) for p in packets] == WANT[name]["pictures"]
    assert [S.frame_hash(r) for r in recs] == WANT[name]["recon"]


@pytest.mark.parametrize("w,h,hdr,bframes,n", [(1920, 1080, False, 0, 6), (3840, 2160, True, 1, 5)])
def test_full_size_session_decodes_to_its_reconstruction(lib, w, h, hdr, bframes, n):
    """the session's defaults (rate control, pre-search, scene cuts, P tiles) with sign hiding; 2160p Main10 with B pictures"""
    from hevc_amd.encoder import Encoder
    cfg, _ = operating_point(w, h, hdr, n)
    cfg.sign_hide, cfg.bframes, cfg.keyint = 1, bframes, 4
    frames = clip_frames(w, h, cfg.bit_depth, n)
    with Encoder(cfg, device=0, keep_recon=True) as enc:
        for (y, u, v), _ in frames:
            enc.send(y, u, v)
        enc.flush()
        stream = b"".join(d for d, _pts, _key in enc.packets())
        recs = [O.Frame(*enc.recon(i)) for i in range(n)]
        types = [enc.frame_info(i)[1] for i in range(n)]
    dec, info = O.decode(stream)
    assert len(dec) == n
    for i in range(n):
        assert dec[i].same(recs[i]), f"display picture {i} (slice type {types[i]}): decoded != session reconstruction"
    assert (0 in types) == bool(bframes)


def test_2160p_as_two_halo_slices_decodes_to_the_reconstruction(lib):
    from hevc_amd.encoder import SlicedEncoder
    n = 4
    cfg, _ = operating_point(3840, 2160, False, n)
    cfg.sign_hide = 1
    frames = clip_frames(3840, 2160, 8, n)
    sl = SlicedEncoder(cfg, [0, 0], keep_recon=True)
    try:
        assert sl.halo
        got = []
        for (y, u, v), _ in frames:
            sl.send(y, u, v)
            got += sl.ready()
        got += sl.finish()
        recs = [O.Frame(*sl.recon(i)) for i in range(n)]
    finally:
        sl.close()
    dec, info = O.decode(b"".join(d for d, _, _ in got))
    assert len(dec) == n and info["count.slices"] == 2 * n
    for i in range(n):
        assert dec[i].same(recs[i]), f"picture {i}: decoded != sliced reconstruction"
