"""GPU (-m gpu): the lane groups of a chunk (hevc_amd/csrc/session.cpp encode_chunk) change the schedule and nothing else.  From step 1 on a
session runs the lanes of a step as two launch sequences on two streams; MIHEVC_LANE_GROUPS=1, read when a session is opened, keeps the single sequence.
Every case codes one clip with the switch at 1 and at 2 and wants the same packets (bytes, pts, dts, key flag), the same headers, the same QP, type and
size of every picture (mihevc_get_frame_info) and the same quality records (mihevc_get_frame_quality), with rate control on wherever the case allows it:
the controller's inputs arrive at fixed lags, and each group has to keep them."""
import functools

import pytest

from tests import util

pytestmark = pytest.mark.gpu

SWITCH = "MIHEVC_LANE_GROUPS"


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


@functools.lru_cache(maxsize=None)
def clip(w, h, bd, n, cut=None):
    """n pictures of a translating scene; cut: another scene from that picture on (tests/test_gpu_ssim.py clip: enough of a jump for the cut detector at 416x240)"""
    if cut is None:
        return tuple(util.synth_frame(h, w, seed=4, shift=(2 * i, i), bit_depth=bd) for i in range(n))
    return tuple(util.synth_frame(h, w, seed=40 + (i >= cut), shift=(i, i // 2), bit_depth=bd) for i in range(n))


def make_cfg(w, h, bd=8, rc=None, **kw):
    """rc: (vbv_maxrate_kbps, vbv_bufsize_kbits) at CRF 20, or None for a fixed QP of 30"""
    from hevc_amd import _lib
    cfg = _lib.default_config()
    cfg.width, cfg.height, cfg.bit_depth, cfg.min_keyint, cfg.scenecut, cfg.me_range, cfg.level_idc, cfg.aud = w, h, bd, 2, 0, 12, 93, 1
    if rc:
        cfg.crf, cfg.qp, cfg.vbv_maxrate_kbps, cfg.vbv_bufsize_kbits, cfg.hrd = 20, -1, rc[0], rc[1], 1
    else:
        cfg.qp = 30
    if bd == 10:      # Main10 HDR10
        cfg.colour_primaries, cfg.transfer, cfg.matrix, cfg.hdr10, cfg.repeat_headers, cfg.hrd, cfg.chroma_loc = 9, 16, 9, 1, 1, 1, 0
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def encode(cfg, frames, keep_recon=False):
    """everything a session says about the clip"""
    from hevc_amd.encoder import Encoder
    n = len(frames)
    with Encoder(cfg, device=0, keep_recon=keep_recon) as enc:
        packets = []
        for f in frames:
            enc.send(*util.planes(f, cfg.bit_depth))
            packets += list(enc.packets_dts())
        enc.flush()
        packets += list(enc.packets_dts())
        st = enc.stats()
        return dict(split_steps=st.reserved[6], packets=packets, headers=enc.headers(), info=[enc.frame_info(i) for i in range(n)], quality=[enc.frame_quality(i) for i in range(n)],
                    totals=(st.frames_out, st.bytes_out, st.sse_y, st.sse_u, st.sse_v, st.ssim_y, st.ssim_u, st.ssim_v),
                    recon=[[p.tobytes() for p in enc.recon(i)] for i in range(n)] if keep_recon else None)


def both(monkeypatch, cfg, frames, keep_recon=False):
    """the clip with the switch at 1 and at 2 -> the (equal) result"""
    out = []
    for groups in ("1", "2"):
        monkeypatch.setenv(SWITCH, groups)
        out.append(encode(cfg, frames, keep_recon))
    one, two = out
    n = len(frames)
    assert one["split_steps"] == 0 and two["split_steps"] > 0, "the switch did not choose the schedule (is another session open on the device?)"
    assert len(one["packets"]) == n and len(two["packets"]) == n
    for i, (a, b) in enumerate(zip(one["packets"], two["packets"])):
        assert a[1:] == b[1:], f"packet {i}: pts / key / dts {a[1:]} != {b[1:]}"
        assert a[0] == b[0], f"packet {i} (pts {a[1]}): {len(a[0])} bytes with one group, {len(b[0])} with two, or other bytes"
    assert one["headers"] == two["headers"]
    assert one["info"] == two["info"], "QP, type or size of a picture depends on the grouping"
    assert one["quality"] == two["quality"]
    assert one["totals"] == two["totals"]
    assert one["recon"] == two["recon"]
    return two


def gop_starts(res):
    return [i for i, (_, t, _) in enumerate(res["info"]) if t == 2]


def p_qps(res):
    return [q for q, t, _ in res["info"] if t == 1]


def test_rate_control_four_equal_gops(lib, monkeypatch):
    """four lanes of 12 pictures, longer than the ring (8 slots): the CABAC sizes of step t - 7 and the estimates of step t - 2 both reach the controller"""
    res = both(monkeypatch, make_cfg(256, 144, rc=(250, 300), keyint=12, gops_in_flight=4), clip(256, 144, 8, 48))
    assert gop_starts(res) == [0, 12, 24, 36]
    assert len(set(p_qps(res))) > 1, "the cap never moved a QP: the feedback path is not exercised"


def test_three_gops_odd_lane_count(lib, monkeypatch):
    res = both(monkeypatch, make_cfg(256, 144, rc=(250, 300), keyint=10, gops_in_flight=3), clip(256, 144, 8, 30))
    assert gop_starts(res) == [0, 10, 20]
    assert len(set(p_qps(res))) > 1


def test_unequal_gops_lanes_drop_out(lib, monkeypatch):
    """a scene cut at picture 5 of 20 (keyint 8): GOPs of unequal length in one chunk, so lanes run out at different steps and the groups shrink"""
    res = both(monkeypatch, make_cfg(416, 240, rc=(600, 720), keyint=8, gops_in_flight=3, scenecut=1), clip(416, 240, 8, 20, cut=5))
    starts = gop_starts(res)
    assert 5 in starts and len(starts) >= 3, starts
    assert len({b - a for a, b in zip(starts, starts[1:] + [20])}) > 1, starts


def test_more_than_one_chunk(lib, monkeypatch):
    """chunks of 2 x 6 pictures: two whole chunks and a last one of a single GOP (one lane: one launch sequence)"""
    res = both(monkeypatch, make_cfg(256, 144, rc=(250, 300), keyint=6, gops_in_flight=2), clip(256, 144, 8, 30))
    assert gop_starts(res) == [0, 6, 12, 18, 24]


def test_b_pictures(lib, monkeypatch):
    res = both(monkeypatch, make_cfg(256, 144, rc=(250, 300), keyint=9, gops_in_flight=4, bframes=1), clip(256, 144, 8, 36))
    assert 0 in [t for _, t, _ in res["info"]]


def test_main10(lib, monkeypatch):
    """Main10, and level 5: the long ring"""
    res = both(monkeypatch, make_cfg(256, 144, 10, rc=(250, 300), keyint=6, gops_in_flight=4, level_idc=150), clip(256, 144, 10, 24))
    assert gop_starts(res) == [0, 6, 12, 18]


@pytest.mark.parametrize("pic_hash", [1, 2])
def test_picture_hash_and_ssim(lib, monkeypatch, pic_hash):
    """the copy stream's passes (hash or the MD5 copy, SSIM) of both groups share one scratch buffer each"""
    res = both(monkeypatch, make_cfg(256, 144, keyint=5, gops_in_flight=4, pic_hash=pic_hash, ssim=1), clip(256, 144, 8, 20))
    assert all(q["ssim"] is not None and 0 < q["ssim"][0] <= 1 for q in res["quality"])


def test_keep_recon(lib, monkeypatch):
    res = both(monkeypatch, make_cfg(256, 144, rc=(250, 300), keyint=5, gops_in_flight=3), clip(256, 144, 8, 15), keep_recon=True)
    assert res["recon"] is not None and len(res["recon"]) == 15


def test_p_tiles(lib, monkeypatch):
    from hevc_amd import _lib
    cfg = make_cfg(512, 64, keyint=4, gops_in_flight=4, p_tiles=1, level_idc=120)
    assert _lib.p_tile_grid(cfg) == (2, 1)
    both(monkeypatch, cfg, clip(512, 64, 8, 16))


def test_sliced_session_runs_and_matches(lib, monkeypatch):
    """slices that exchange rows keep one launch sequence whatever the switch says: the same access units either way"""
    from hevc_amd.encoder import SlicedEncoder
    w, h, n = 160, 160, 10
    frames = clip(w, h, 8, n)
    out = []
    for groups in ("1", "2"):
        monkeypatch.setenv(SWITCH, groups)
        cfg = make_cfg(w, h, rc=(400, 480), keyint=5, gops_in_flight=2, hrd=0)
        sl = SlicedEncoder(cfg, [0, 0], keep_recon=True)
        try:
            assert sl.halo
            got = []
            for f in frames:
                sl.send(*util.planes(f, 8))
                got += sl.ready()
            got += sl.finish()
            out.append((got, [[e.frame_info(i) for i in range(n)] for e in sl._encs], [[p.tobytes() for p in sl.recon(i)] for i in range(n)]))
            assert all(st.reserved[6] == 0 for st in sl.stats()), "slices that exchange rows keep one launch sequence"
        finally:
            sl.close()
    assert len(out[0][0]) == n
    assert out[0] == out[1]
