"""GPU (-m gpu): the learned super-resolution path on an MI355X.  1. k_sr_conv alone (mihevc_k_sr_conv) bit for bit against the integer numpy
convolution over every case of the stepped tests: this is what proves the MFMA lane maps; 2. k_sr_input alone against numpy; 3. the whole network
(mihevc_k_sr_network) against the float64 model within twice the half model's own error plus half a unit of half precision at 1.0, over every output element;
the eight cases with the initialisation's weights hold the last layers and the plumbing, the four with plain Kaiming weights are the ones a missing or
mis-wired trunk launch fails (tests/sr_common.py NET_CASES, tests/test_sr_cpu.py test_the_bound_sees_every_part_of_the_network);
4. sessions: the stream of send_sr is byte for byte that of a plain session fed the network's half planes through send_rgb, decodes to the reconstruction, is
the same from host planes, device planes and a torch tensor (child process), follows a model replaced between frames, and every refusal leaves it usable; 5. encode_file(sr_model=) over a stand-in ffmpeg pipe.

Measured on an MI355X (E_h = max |Mh - M64|, E_dev = max |device - M64|, bound = 2 E_h + 2^-11): DESIGN.md §6l has the table."""
import ctypes as C
import functools
import hashlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import sr_common as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


# ------------------------------------------------------------------------------------------------ 1. the convolution, exactly
@pytest.mark.parametrize("case_id", S.CONV_IDS)
def test_conv_is_exact(lib, case_id):
    """the slice the launch writes equals the integer convolution bit for bit; everything else in the output buffer is as it was"""
    out, want = S.run_conv(lib, "mihevc_k_", case_id, device=0)
    assert np.array_equal(out, want), np.argwhere(out != want)[:5]


def test_conv_is_deterministic(lib):
    a, _ = S.run_conv(lib, "mihevc_k_", "conv5-40x24", device=0)
    b, _ = S.run_conv(lib, "mihevc_k_", "conv5-40x24", device=0)
    assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 2. the input kernel
@pytest.mark.parametrize("scale", [4, 2])
@pytest.mark.parametrize("name", S.INPUT_FORMATS)
def test_input_is_numpys(lib, name, scale):
    assert np.array_equal(S.run_input(lib, "mihevc_k_", name, scale, device=0), S.input_want(name, scale))


# ------------------------------------------------------------------------------------------------ 3. the whole network
@pytest.mark.parametrize("case", S.NET_CASES, ids=S.net_id)
def test_network_is_within_twice_the_half_models_error(lib, case):
    dev = S.run_network(lib, "mihevc_k_", case, device=0)
    e_h, e_dev, bound = S.network_errors(dev, case)
    print(f"SR_ERRORS {S.net_id(case)}: E_h {e_h:.4e}  E_dev {e_dev:.4e}  bound {bound:.4e}")
    assert np.isfinite(dev.astype(np.float32)).all() and 0 < e_h
    assert e_dev <= bound


def test_network_is_deterministic(lib):
    a = S.run_network(lib, "mihevc_k_", S.NET_CASES[1], device=0)
    b = S.run_network(lib, "mihevc_k_", S.NET_CASES[1], device=0)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))


# ------------------------------------------------------------------------------------------------ 4. sessions
def drain(enc):
    enc.flush()
    return b"".join(d for d, _, _ in enc.packets())


@functools.lru_cache(maxsize=None)
def reference_stream(scale, depth, models=(0, 0, 0, 0)):
    """the stream of a plain session fed, through send_rgb, the half planes mihevc_k_sr_network returns for every source; models: the seed of each picture's model"""
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    L = _lib.load()
    half = _lib.RgbFormat(*S.HALF_PLANES)
    with Encoder(S.session_cfg(depth), device=0) as enc:
        for planes, seed in zip(S.session_clip(scale, depth), models):
            out = S.network_planes(L, S.session_model(scale, seed), S.session_format(depth), planes)
            enc.send_rgb(half, *[np.ascontiguousarray(p).view(np.float16) for p in out])
        return drain(enc)


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("scale", [4, 2])
def test_session_stream_equals_the_network_fed_session(lib, scale, depth):
    from hevc_amd.encoder import Encoder
    from oracle import oracle as O
    want = reference_stream(scale, depth)
    sw, sh = S.SESSION_W // scale, S.SESSION_H // scale
    for route in ("sync", "async"):
        keep = []
        with Encoder(S.session_cfg(depth), device=0, keep_recon=True) as enc:
            enc.set_sr_model(S.session_model(scale))
            for planes in S.session_clip(scale, depth):
                keep.append(planes)
                enc.send_sr(S.session_format(depth), sw, sh, *planes, asynchronous=route == "async")
            got = drain(enc)
            recs = [O.Frame(*enc.recon(i)) for i in range(S.SESSION_N)]
        assert len(want) > 400 and got == want, route
    dec, _ = O.decode(got)
    assert len(dec) == S.SESSION_N and all(d.same(r) for d, r in zip(dec, recs))


def test_the_network_changes_the_picture(lib):
    """the reference stream is not the stream of a flat picture: the half planes carry the source (enlarged) and differ between pictures.  The random layers
    beside the copying path give the picture a gain and an offset nobody predicts, so the check is the correlation with the source, not a distance"""
    from hevc_amd import _lib
    a, b = [S.network_planes(lib, S.session_model(4), S.session_format(8), p).view(np.float16).astype(np.float32) for p in S.session_clip(4, 8)[:2]]
    src = np.asarray(S.session_clip(4, 8)[0][2], np.float32) / 255          # R
    assert np.ptp(a[0]) > 0.3 and np.abs(a - b).max() > 0.05
    assert np.corrcoef(a[0][::4, ::4].reshape(-1), src.reshape(-1))[0, 1] > 0.9


@pytest.fixture(scope="module")
def device_streams():
    """SHA-256 of the streams of sessions fed from torch tensors, from ONE child process in which torch is initialised before the library
    (tests/sr_device_child.py says why): what this test is about is that order"""
    p = subprocess.run([sys.executable, "-s", "-m", "tests.sr_device_child"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    return json.loads(p.stdout[p.stdout.index("{"):])


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("scale", [4, 2])
def test_device_planes_and_tensors_give_the_same_stream(lib, device_streams, scale, depth):
    want = hashlib.sha256(reference_stream(scale, depth)).hexdigest()
    assert device_streams[f"planes-x{scale}-{depth}"] == want
    if depth == 8:
        assert device_streams[f"tensor-x{scale}-{depth}"] == want


def test_a_model_replaced_between_frames_takes_effect_at_the_next_frame(lib):
    from hevc_amd.encoder import Encoder
    models = (0, 0, 1, 1)
    want = reference_stream(4, 8, models)
    with Encoder(S.session_cfg(8), device=0) as enc:
        for i, (planes, seed) in enumerate(zip(S.session_clip(4, 8), models)):
            if i == 0 or models[i - 1] != seed:
                enc.set_sr_model(S.session_model(4, seed))
            enc.send_sr(S.session_format(8), 48, 32, *planes, asynchronous=True)      # nothing waits between the frames and the new model
        got = drain(enc)
    assert got == want and want != reference_stream(4, 8)


def test_refusals_leave_the_session_usable(lib):
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    fmt = S.session_format(8)
    clip = S.session_clip(4, 8)
    model = S.session_model(4)

    def send(enc, f, w, h, planes, pitch=None, flags=0):
        p = [None if q is None else q.ctypes.data for q in planes]
        return lib.mihevc_send_frame_sr(enc._s, None if f is None else C.byref(f), w, h, *p, w if pitch is None else pitch, 99, flags)

    big = [np.zeros((130, 200), np.uint8)] * 3
    with Encoder(S.session_cfg(8), device=0) as enc:
        assert send(enc, fmt, 48, 32, clip[0]) == _lib.EINVAL                        # no model set
        m = _lib.SrModel(4, 1)
        w = model.weights
        assert lib.mihevc_set_sr_model(enc._s, C.byref(_lib.SrModel(3, 1)), w.ctypes.data, w.size) == _lib.EINVAL
        assert lib.mihevc_set_sr_model(enc._s, C.byref(m), w.ctypes.data, w.size - 1) == _lib.EINVAL
        assert lib.mihevc_set_sr_model(enc._s, C.byref(m), None, w.size) == _lib.EINVAL
        assert send(enc, fmt, 48, 32, clip[0]) == _lib.EINVAL                        # still none
        for i, planes in enumerate(clip):
            if i == 0:
                enc.set_sr_model(model)
            if i == 2:
                assert send(enc, None, 48, 32, planes) == _lib.EINVAL
                for sw, sh in ((47, 32), (48, 33), (96, 64), (3, 32), (48, 3)):      # a size mismatch, sides below 4
                    assert send(enc, fmt, sw, sh, big, 200) == _lib.EINVAL, (sw, sh)
                bad = _lib.RgbFormat.from_buffer_copy(bytes(fmt))
                bad.layout = 2
                assert send(enc, bad, 48, 32, planes) == _lib.EINVAL
                bad = _lib.RgbFormat.from_buffer_copy(bytes(fmt))
                bad.matrix = 2
                assert send(enc, bad, 48, 32, planes) == _lib.EINVAL
                assert send(enc, fmt, 48, 32, planes, pitch=47) == _lib.EINVAL and send(enc, fmt, 48, 32, planes, flags=4) == _lib.EINVAL
                assert send(enc, fmt, 48, 32, [planes[0], None, planes[2]]) == _lib.EINVAL
                enc.set_sr_model(None)                                               # dropped: refused; set again: goes on
                assert send(enc, fmt, 48, 32, planes) == _lib.EINVAL
                enc.set_sr_model(model)
            enc.send_sr(fmt, 48, 32, *planes)
        stream = drain(enc)
        assert send(enc, fmt, 48, 32, clip[0]) == _lib.ESTATE
    assert stream == reference_stream(4, 8)
    # scale 2 takes no odd source: a 194x130 session would fit 97x65
    cfg = S.session_cfg(8)
    cfg.width, cfg.height = 194, 130
    with Encoder(cfg, device=0) as enc:
        enc.set_sr_model(S.session_model(2))
        assert send(enc, fmt, 97, 65, big, 200) == _lib.EINVAL
    # one band of a picture coded as two slices takes neither a model nor a frame
    cfg = S.session_cfg(8)
    cfg.height, cfg.pic_height, cfg.slice_count, cfg.slice_index = 64, 128, 2, 0
    cfg.slice_ctu_rows[0], cfg.slice_ctu_rows[1] = 2, 2
    cfg.rate_share_q16 = 32768
    with Encoder(cfg, device=0) as enc:
        assert lib.mihevc_set_sr_model(enc._s, C.byref(_lib.SrModel(4, 1)), model.weights.ctypes.data, model.weights.size) == _lib.EINVAL
        assert send(enc, fmt, 48, 16, clip[0]) == _lib.EINVAL


# ------------------------------------------------------------------------------------------------ 5. encode_file
def test_encode_file_with_a_model_over_the_pipe(lib, tmp_path, monkeypatch):
    """a stand-in ffmpeg that answers the rawvideo request with frames of zeros: the clip is asked for as gbrp, the session, its level and the MP4 track open at
    4 x the source size, every picture goes through send_sr, and the stream is that of a session of the same configuration fed the same pictures by hand; it
    decodes to the session's reconstruction"""
    from hevc_amd import _lib, encoder, mp4, probe
    from hevc_amd.transcoder import calculate_apple_hevc_level
    from oracle import oracle as O
    from tests.test_host_robustness import FAKE_FFMPEG
    sw, sh, n = 48, 32, 4
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
        """the session of encode_file, keeping its reconstructions and what it put out"""
        def __init__(self, cfg, device=0):
            super().__init__(cfg, device=device, keep_recon=True)
            self.stream = b""
            seen.append(self)

        def packets_dts(self):
            for data, pts, key, dts in super().packets_dts():
                self.stream += data
                yield data, pts, key, dts

        def close(self):
            if self._s:
                self.recs = [self.recon(i) for i in range(n)]
            super().close()

    monkeypatch.setattr(encoder, "Encoder", Keeping)
    info = probe.VideoInfo(sw, sh, 30.0, "bt709", "bt709", "gbr", "gbrp", "", "", 0, False, "eng", n, n / 30.0)
    out = tmp_path / "restored.mp4"
    model = S.session_model(4)
    assert encoder.encode_file(tmp_path / "scan.mkv", out, info, total_frames=n, device=0, sr_model=model) == 0
    argv = (tmp_path / "ffmpeg.log").read_text().split("\n")[0].split()
    assert argv[argv.index("-pix_fmt") + 1] == "gbrp" and not {"-s", "-vf", "-filter:v"} & set(argv)
    (enc,) = seen
    assert (enc.cfg.width, enc.cfg.height) == (4 * sw, 4 * sh)
    big = probe.VideoInfo(4 * sw, 4 * sh, 30.0, "bt709", "bt709", "gbr", "gbrp", "", "", 0, False, "eng", n, n / 30.0)
    assert enc.cfg.level_idc == int(round(float(calculate_apple_hevc_level(big)[0]) * 30))      # the level follows the enlarged size
    dec, _ = O.decode(enc.stream)
    assert len(dec) == n and all(d.same(O.Frame(*r)) for d, r in zip(dec, enc.recs))
    zeros = [np.zeros((sh, sw), np.uint8)] * 3
    with RealEncoder(type(enc.cfg).from_buffer_copy(bytes(enc.cfg)), device=0) as ref:
        ref.set_sr_model(model)
        want = b""
        for i in range(n):
            ref.send_sr(_lib.rgb_format_for("gbrp"), sw, sh, *zeros, pts=i)
            want += b"".join(d for d, _, _ in ref.packets())
        ref.flush()
        want += b"".join(d for d, _, _ in ref.packets())
    assert len(want) > 100 and enc.stream == want
    data = out.read_bytes()
    start, end = 0, len(data)
    for name in ("moov", "trak", "tkhd"):
        _, start, end = [x for x in mp4.parse_boxes(data, start, end) if x[0] == name][0]
    assert (int.from_bytes(data[end - 8:end - 4], "big") >> 16, int.from_bytes(data[end - 4:end], "big") >> 16) == (4 * sw, 4 * sh)      # the track has the enlarged size
    start, end = 0, len(data)
    for name in ("moov", "trak", "mdia", "minf", "stbl", "stsz"):
        _, start, end = [x for x in mp4.parse_boxes(data, start, end) if x[0] == name][0]
    assert int.from_bytes(data[start + 8:start + 12], "big") == n
