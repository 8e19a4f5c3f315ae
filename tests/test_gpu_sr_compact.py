"""GPU (-m gpu): compact super-resolution networks on an MI355X.  1. k_sr_compact alone (mihevc_k_sr_compact_conv) bit for bit against the
integer numpy convolutions over every case of the stepped tests and one with more tiles than workgroups: this is what proves the MFMA lane maps and the
shuffled stores; 2. the whole network (mihevc_k_sr_compact_network) against the float64 model within twice the half model's own error plus half a unit of half
precision at 1.0, over every output element (tests/test_sr_compact_cpu.py shows that the bound sees every defect the cases exist for); 3. sessions: the stream
of send_sr / send_sr_yuv / send_sr_fit under a compact model is byte for byte that of a plain session fed the network's half planes by hand, decodes to the
reconstruction, follows a model of the other kind set between frames, takes odd sources at scale 2, and every refusal leaves it usable; 4.
encode_file(sr_model=(a, b), sr_denoise=) over a stand-in ffmpeg pipe.

Measured on an MI355X (E_h = max |Mh - M64|, E_dev = max |device - M64|, bound = 2 E_h + 2^-11): DESIGN.md §6m has the table."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import sr_common as S
from tests import sr_compact_common as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


# ------------------------------------------------------------------------------------------------ 1. the convolution, exactly
@pytest.mark.parametrize("case_id", K.CONV_IDS)
def test_conv_is_exact(lib, case_id):
    out, want = K.run_conv(lib, "mihevc_k_", case_id, device=0)
    assert np.array_equal(out, want), np.argwhere(out != want)[:5]


def test_conv_is_deterministic(lib):
    a, _ = K.run_conv(lib, "mihevc_k_", "tail4-37x35", device=0)
    b, _ = K.run_conv(lib, "mihevc_k_", "tail4-37x35", device=0)
    assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 2. the whole network
@pytest.mark.parametrize("case", K.NET_CASES, ids=K.net_id)
def test_network_is_within_twice_the_half_models_error(lib, case):
    dev = K.run_network(lib, "mihevc_k_", case, device=0)
    e_h, e_dev, bound = K.network_errors(dev, case)
    print(f"SR_COMPACT_ERRORS {K.net_id(case)}: E_h {e_h:.4e}  E_dev {e_dev:.4e}  bound {bound:.4e}")
    assert np.isfinite(dev.astype(np.float32)).all() and 0 < e_h
    assert e_dev <= bound


def test_network_is_deterministic(lib):
    a = K.run_network(lib, "mihevc_k_", K.NET_CASES[6], device=0)
    b = K.run_network(lib, "mihevc_k_", K.NET_CASES[6], device=0)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))


# ------------------------------------------------------------------------------------------------ 3. sessions
def drain(enc):
    enc.flush()
    return b"".join(d for d, _, _ in enc.packets())


def planes_of(lib, model, fmt, planes):
    """the half planes of a source under a model of either kind"""
    return (K if hasattr(model, "convs") else S).network_planes(lib, model, fmt, planes)


def by_hand(lib, cfg, halves):
    """the stream of a plain session fed the network's half planes of every picture through send_rgb"""
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    with Encoder(cfg, device=0) as enc:
        for half in halves:
            enc.send_rgb(_lib.RgbFormat(*S.HALF_PLANES), *[np.ascontiguousarray(p).view(np.float16) for p in half])
        return drain(enc)


def model_of(kind, scale):
    return K.session_model(scale) if kind == "compact" else S.session_model(scale)


@functools.lru_cache(maxsize=None)
def reference_stream(scale, depth, kinds=("compact",) * S.SESSION_N):
    """kinds: per picture, the kind of session model it is sent under: 'compact' or 'rrdb'"""
    from hevc_amd import _lib
    L = _lib.load()
    return by_hand(L, S.session_cfg(depth), [planes_of(L, model_of(k, scale), S.session_format(depth), p) for p, k in zip(S.session_clip(scale, depth), kinds)])


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("scale", [4, 2])
def test_session_stream_equals_the_network_fed_session(lib, scale, depth):
    from hevc_amd.encoder import Encoder
    from oracle import oracle as O
    want = reference_stream(scale, depth)
    sw, sh = S.SESSION_W // scale, S.SESSION_H // scale
    for route in ("sync", "async"):
        with Encoder(S.session_cfg(depth), device=0, keep_recon=True) as enc:
            enc.set_sr_model(K.session_model(scale))
            for planes in S.session_clip(scale, depth):
                enc.send_sr(S.session_format(depth), sw, sh, *planes, asynchronous=route == "async")
            got = drain(enc)
            recs = [O.Frame(*enc.recon(i)) for i in range(S.SESSION_N)]
        assert len(want) > 400 and got == want, route
    dec, _ = O.decode(got)
    assert len(dec) == S.SESSION_N and all(d.same(r) for d, r in zip(dec, recs))


def test_the_network_changes_the_picture(lib):
    a, b = [K.network_planes(lib, K.session_model(4), S.session_format(8), p).view(np.float16).astype(np.float32) for p in S.session_clip(4, 8)[:2]]
    src = np.asarray(S.session_clip(4, 8)[0][2], np.float32) / 255          # R
    near = src.repeat(4, axis=0).repeat(4, axis=1)
    assert np.ptp(a[0]) > 0.3 and np.abs(a - b).max() > 0.05
    assert np.abs(a[0] - near).max() > 0.02          # not the bare enlargement either: the layers add their texture
    assert np.corrcoef(a[0].reshape(-1), near.reshape(-1))[0, 1] > 0.9


@pytest.mark.parametrize("order", ["rrdb-then-compact", "compact-then-rrdb"])
def test_a_model_of_the_other_kind_takes_effect_at_the_next_frame(lib, order):
    from hevc_amd.encoder import Encoder
    pair = ("rrdb", "compact") if order == "rrdb-then-compact" else ("compact", "rrdb")
    kinds = (pair[0], pair[0], pair[1], pair[1])
    want = reference_stream(4, 8, kinds)
    with Encoder(S.session_cfg(8), device=0) as enc:
        for i, (planes, k) in enumerate(zip(S.session_clip(4, 8), kinds)):
            if i == 0 or kinds[i - 1] != k:
                enc.set_sr_model(model_of(k, 4))
            enc.send_sr(S.session_format(8), 48, 32, *planes, asynchronous=True)      # nothing waits between the frames and the new model
        got = drain(enc)
    assert got == want and want != reference_stream(4, 8)


def test_yuv_stream_equals_the_hand_fed_one(lib):
    from hevc_amd.encoder import Encoder
    from tests import sr_yuv_common as Q
    sw, sh = 48, 32
    clip = Q.yuv_clip(sw, sh, 8)
    with Encoder(Q.session_cfg(8), device=0) as enc:
        enc.set_sr_model(K.session_model(4))
        for planes in clip:
            enc.send_sr_yuv(sw, sh, *planes, bit_depth=8, matrix=6)
        got = drain(enc)
    halves = [K.network_planes(lib, K.session_model(4), *Q.rgb16_planes(p, 8, 6, False)) for p in clip]
    want = by_hand(lib, Q.session_cfg(8), halves)
    assert len(want) > 400 and got == want


def test_fit_stream_equals_the_hand_fed_one(lib):
    """48x32 x4 = 192x128 into a 108x72 session: the resized route behind a compact model"""
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    from tests import sr_yuv_common as Q
    cfg = Q.session_cfg(8, 108, 72)
    gbrp = _lib.rgb_format_for("gbrp")
    clip = S.session_clip(4, 8)
    with Encoder(Q.session_cfg(8, 108, 72), device=0) as enc:
        enc.set_sr_model(K.session_model(4))
        for planes in clip:
            enc.send_sr_fit(gbrp, 48, 32, *planes)
        got = drain(enc)
    with Encoder(cfg, device=0) as enc:
        for planes in clip:
            half = K.network_planes(lib, K.session_model(4), gbrp, planes)
            enc.send_scaled(192, 128, *Q.intermediate_planes(lib, half, cfg.matrix, bool(cfg.full_range)), bit_depth=10)
        want = drain(enc)
    assert len(want) > 300 and got == want


def test_an_odd_source_with_a_scale_2_model(lib):
    """97x65 into 194x130: a compact network has no pixel-unshuffle"""
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    from tests import util
    cfg = S.session_cfg(8)
    cfg.width, cfg.height = 194, 130
    gbrp = _lib.rgb_format_for("gbrp")
    clip = []
    for i in range(3):
        y = np.asarray(util.synth_frame(72, 104, seed=5, shift=(2 * i, i), bit_depth=8).y)[:65, :97].astype(np.uint8)
        clip.append([np.ascontiguousarray(y), np.ascontiguousarray(y[::-1]), np.ascontiguousarray(y[:, ::-1])])
    with Encoder(cfg, device=0) as enc:
        enc.set_sr_model(K.session_model(2))
        for planes in clip:
            enc.send_sr(gbrp, 97, 65, *planes)
        got = drain(enc)
    want = by_hand(lib, cfg, [K.network_planes(lib, K.session_model(2), gbrp, p) for p in clip])
    assert len(want) > 300 and got == want


def test_refusals_leave_the_session_usable(lib):
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    fmt = S.session_format(8)
    clip = S.session_clip(4, 8)
    model = K.session_model(4)
    w = model.weights

    def send(enc, f, sw, sh, planes, pitch=None, flags=0):
        p = [None if q is None else q.ctypes.data for q in planes]
        return lib.mihevc_send_frame_sr(enc._s, None if f is None else C.byref(f), sw, sh, *p, sw if pitch is None else pitch, 99, flags)

    def set_compact(enc, m, weights=w, count=None):
        return lib.mihevc_set_sr_compact(enc._s, None if m is None else C.byref(m), None if weights is None else weights.ctypes.data, w.size if count is None else count)

    big = [np.zeros((130, 200), np.uint8)] * 3
    good = _lib.SrCompact(4, K.SESSION_CONVS)
    with Encoder(S.session_cfg(8), device=0) as enc:
        assert send(enc, fmt, 48, 32, clip[0]) == _lib.EINVAL                        # no model set
        reserved = _lib.SrCompact(4, K.SESSION_CONVS)
        reserved.reserved[0] = 1
        for bad in (None, _lib.SrCompact(3, K.SESSION_CONVS), _lib.SrCompact(4, 0), _lib.SrCompact(4, 65), _lib.SrCompact(2, K.SESSION_CONVS), reserved):
            assert set_compact(enc, bad) == _lib.EINVAL
        assert set_compact(enc, good, count=w.size - 1) == set_compact(enc, good, count=w.size + 1) == set_compact(enc, good, weights=None) == _lib.EINVAL
        assert send(enc, fmt, 48, 32, clip[0]) == _lib.EINVAL                        # still none
        for i, planes in enumerate(clip):
            if i == 0:
                assert set_compact(enc, good) == 0
            if i == 2:
                assert send(enc, None, 48, 32, planes) == _lib.EINVAL
                for sw, sh in ((47, 32), (48, 33), (96, 64), (3, 32), (48, 3)):      # a size mismatch, sides below 4
                    assert send(enc, fmt, sw, sh, big, 200) == _lib.EINVAL, (sw, sh)
                assert send(enc, fmt, 48, 32, planes, pitch=47) == _lib.EINVAL and send(enc, fmt, 48, 32, planes, flags=4) == _lib.EINVAL
                enc.set_sr_model(None)                                               # set_sr_model(None) drops a compact model too
                assert send(enc, fmt, 48, 32, planes) == _lib.EINVAL
                enc.set_sr_model(model)
            enc.send_sr(fmt, 48, 32, *planes)
        stream = drain(enc)
        assert send(enc, fmt, 48, 32, clip[0]) == _lib.ESTATE
    assert stream == reference_stream(4, 8)
    # one band of a picture coded as two slices takes neither a model nor a frame
    cfg = S.session_cfg(8)
    cfg.height, cfg.pic_height, cfg.slice_count, cfg.slice_index = 64, 128, 2, 0
    cfg.slice_ctu_rows[0], cfg.slice_ctu_rows[1] = 2, 2
    cfg.rate_share_q16 = 32768
    with Encoder(cfg, device=0) as enc:
        assert set_compact(enc, good) == _lib.EINVAL
        assert send(enc, fmt, 48, 16, clip[0]) == _lib.EINVAL


# ------------------------------------------------------------------------------------------------ 4. encode_file
def test_encode_file_blends_a_pair_by_sr_denoise(lib, tmp_path, monkeypatch):
    """a stand-in ffmpeg that answers the rawvideo request with frames of zeros; the stream is that of a session given blend(a, b, 0.5) by hand, and a lone
    model with sr_denoise, a pair without it and an RRDBNet in a pair are refused"""
    from hevc_amd import _lib, encoder, probe, sr
    from tests.test_host_robustness import FAKE_FFMPEG
    sw, sh, n = 48, 32, 3
    b = tmp_path / "bin"
    b.mkdir()
    (b / "ffmpeg").write_text(FAKE_FFMPEG)
    (b / "ffmpeg").chmod(0o755)
    monkeypatch.setenv("PATH", f"{b}:/usr/bin:/bin")
    monkeypatch.setenv("FAKE_LOG", str(tmp_path / "ffmpeg.log"))
    monkeypatch.setenv("FAKE_FRAMES", str(n))
    monkeypatch.setenv("FAKE_FB", str(sw * sh * 3))
    seen, RealEncoder = [], encoder.Encoder

    class Keeping(RealEncoder):
        def __init__(self, cfg, device=0):
            super().__init__(cfg, device=device)
            self.stream = b""
            seen.append(self)

        def packets_dts(self):
            for data, pts, key, dts in super().packets_dts():
                self.stream += data
                yield data, pts, key, dts

    monkeypatch.setattr(encoder, "Encoder", Keeping)
    info = probe.VideoInfo(sw, sh, 30.0, "bt709", "bt709", "gbr", "gbrp", "", "", 0, False, "eng", n, n / 30.0)
    ma, mb = K.session_model(4, 0), K.session_model(4, 3)
    run = lambda **kw: encoder.encode_file(tmp_path / "scan.mkv", tmp_path / "out.mp4", info, total_frames=n, device=0, **kw)
    assert run(sr_model=ma, sr_denoise=0.5) == 1 and run(sr_model=(ma, mb)) == 1 and run(sr_model=(ma, S.session_model(4)), sr_denoise=0.5) == 1
    assert run(sr_model=(ma, mb), sr_denoise=1.5) == 1 and run(sr_denoise=0.5) == 1
    assert not seen
    assert run(sr_model=(ma, mb), sr_denoise=0.5) == 0
    (enc,) = seen
    zeros = [np.zeros((sh, sw), np.uint8)] * 3

    def hand(model):
        with RealEncoder(type(enc.cfg).from_buffer_copy(bytes(enc.cfg)), device=0) as ref:
            ref.set_sr_model(model)
            want = b""
            for i in range(n):
                ref.send_sr(_lib.rgb_format_for("gbrp"), sw, sh, *zeros, pts=i)
                want += b"".join(d for d, _, _ in ref.packets())
            ref.flush()
            return want + b"".join(d for d, _, _ in ref.packets())

    want = hand(sr.blend(ma, mb, 0.5))
    assert len(want) > 100 and enc.stream == want
    assert want != hand(ma) and want != hand(mb)          # the blend is neither of its parts
