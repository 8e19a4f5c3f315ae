"""GPU (-m gpu): the upscaling source on an MI355X.  The kernel alone (mihevc_k_upscale_source) against the numpy model of tests/upscale_ref.py,
bit for bit, over the size pairs, depths and settings of the CPU tests, misaligned planes and one 1080p picture; sessions fed smaller sources through
mihevc_send_frame_upscaled (synchronous, asynchronous, device planes) give byte for byte the stream of a session fed the model's output through
mihevc_send_frame; errors leave the session usable; encode_file(upscale=) on a y4m."""
import ctypes as C
import functools
import hashlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import upscale_ref as R
from tests import util
from tests.ingest_common import H, N, W, alignment_class, drain, same_planes, view_of_class
from tests.upscale_common import CASES, SETTINGS, SOURCES, case_id, cfg_of, clip, model, source

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def k_upscale(lib, src, B, dw, dh, D, setting, pitch=None):
    from hevc_amd import _lib
    pw, ph = R.coded(dw), R.coded(dh)
    out = [np.full(s, 0x77, R.out_dtype(D)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    sh, sw = src[0].shape
    pitch = pitch or (sw, sw // 2)
    rc = lib.mihevc_k_upscale_source(0, C.byref(_lib.UpscaleSrc(sw, sh, B, *setting)), *[p.ctypes.data for p in src], pitch[0], pitch[1], dw, dh, D,
                                     *[p.ctypes.data for p in out])
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: f"s{s[0]}a{s[1]}")
@pytest.mark.parametrize("B,D", [(8, 8), (10, 10), (16, 8)])
def test_stage_equals_model(lib, B, D, setting):
    for case in CASES:
        diff = same_planes(k_upscale(lib, source(case, B), B, *case[1], D, setting), model(case, B, D, setting))
        assert not diff, (case_id(case), diff)


@pytest.mark.parametrize("cls", [1, 4, 8])
@pytest.mark.parametrize("B,D", [(8, 8), (16, 8)], ids=["u8", "u16"])
def test_stage_with_misaligned_planes(lib, B, D, cls):
    """the planes' addresses and pitches allow chunks of `cls` bytes and no wider"""
    for case in (CASES[2], CASES[7]):
        views = [view_of_class(p, cls) for p in source(case, B)]
        assert all(alignment_class(v.ctypes.data) == alignment_class(v.strides[0]) == cls for v in views)
        assert views[2].strides == views[1].strides
        pitches = (views[0].strides[0] // views[0].itemsize, views[1].strides[0] // views[1].itemsize)
        diff = same_planes(k_upscale(lib, views, B, *case[1], D, (8, 8), pitches), model(case, B, D, (8, 8)))
        assert not diff, (case_id(case), diff)


def test_stage_equals_model_at_1080p(lib):
    """tile counts and index ranges of a real picture: 960x540 -> 1920x1080, 8 bit"""
    src = R.random_source(960, 540, 8, 7)
    diff = same_planes(k_upscale(lib, src, 8, 1920, 1080, 8, (8, 8)), R.upscale(*src, 8, 1920, 1080, 8, 8, 8))
    assert not diff, diff


# ------------------------------------------------------------------------------------------------ 2. sessions
@functools.lru_cache(maxsize=None)
def reference_stream(size, depth, src_depth=None, settings=((8, 8),) * N):
    """the stream of a session fed the MODEL's pictures, display size, through mihevc_send_frame; settings: (sharpen, antiring) per picture"""
    from hevc_amd.encoder import Encoder
    with Encoder(cfg_of(depth), device=0) as enc:
        for src, st in zip(clip(size, src_depth or depth), settings):
            y, u, v = R.upscale(*src, src_depth or depth, W, H, depth, *st)
            enc.send(y[:H, :W], u[:H // 2, :W // 2], v[:H // 2, :W // 2])
        return drain(enc)


@pytest.mark.parametrize("route", ["sync", "async"])
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("size", SOURCES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_session_stream_equals_the_model_fed_session(lib, size, depth, route):
    from hevc_amd.encoder import Encoder
    want = reference_stream(size, depth)
    keep = []
    with Encoder(cfg_of(depth), device=0) as enc:
        assert enc.coded_size() == (104, 72)
        for src in clip(size, depth):
            keep.append(src)
            enc.send_upscaled(size[0], size[1], *src, asynchronous=route == "async")
        got = drain(enc)
    assert len(want) > 200 and got == want


@pytest.fixture(scope="module")
def device_streams():
    """SHA-256 of the streams of sessions fed from torch tensors (ingest_common.device_planes), from ONE child process in which torch is initialised before the
    library (tests/upscale_device_child.py says why): what this test is about is that order"""
    p = subprocess.run([sys.executable, "-s", "-m", "tests.upscale_device_child"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    return json.loads(p.stdout[p.stdout.index("{"):])


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("size", SOURCES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_session_fed_device_planes_equals_the_model_fed_session(lib, device_streams, size, depth):
    want = reference_stream(size, depth)
    assert len(want) > 200 and device_streams[f"{size[0]}x{size[1]}-{depth}"] == hashlib.sha256(want).hexdigest()


def test_a_deeper_source_is_rounded_once(lib):
    """a 10-bit source into an 8-bit session: the model's 10 -> 8 output, not a pre-rounded source"""
    from hevc_amd.encoder import Encoder
    size = SOURCES[0]
    want = reference_stream(size, 8, 10)
    with Encoder(cfg_of(8), device=0) as enc:
        for src in clip(size, 10):
            enc.send_upscaled(size[0], size[1], *src, bit_depth=10)
        got = drain(enc)
    assert len(want) > 200 and got == want


def test_settings_changed_mid_clip_take_effect_on_their_frame(lib):
    from hevc_amd.encoder import Encoder
    size, depth = SOURCES[1], 8
    settings = ((8, 8), (8, 8), (48, 8), (0, 3), (8, 8))
    want = reference_stream(size, depth, None, settings)
    with Encoder(cfg_of(depth), device=0) as enc:
        for src, (g, ar) in zip(clip(size, depth), settings):
            enc.send_upscaled(size[0], size[1], *src, sharpen=g, antiring=ar)
        got = drain(enc)
    assert len(want) > 200 and got == want and want != reference_stream(size, depth)


# ------------------------------------------------------------------------------------------------ 3. errors
def test_bad_calls_leave_the_session_usable(lib):
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    size, depth = SOURCES[0], 8
    sw, sh = size
    U = _lib.UpscaleSrc
    good = U(sw, sh, depth, 8, 8)

    def send(enc, src, planes, pitch_y=sw, pitch_c=sw // 2, flags=0):
        return lib.mihevc_send_frame_upscaled(enc._s, None if src is None else C.byref(src), *planes, pitch_y, pitch_c, 99, flags)

    big = np.zeros((H + 2) * (W + 2), np.uint8)          # room for every size the refused calls name
    with Encoder(cfg_of(depth), device=0) as enc:
        for i, src in enumerate(clip(size, depth)):
            if i == 2:
                p = [q.ctypes.data for q in src]
                b = [big.ctypes.data] * 3
                assert send(enc, None, p) == _lib.EINVAL
                for bad in (U(sw + 1, sh, depth, 8, 8), U(sw, sh - 1, depth, 8, 8), U(14, sh, depth, 8, 8), U(sw, 14, depth, 8, 8),      # odd, below 16
                            U(W + 2, sh, depth, 8, 8), U(sw, H + 2, depth, 8, 8),                                                        # larger than the session on one axis
                            U(24, sh, depth, 8, 8), U(sw, 16, depth, 8, 8),                                                              # beyond 1:4
                            U(sw, sh, 7, 8, 8), U(sw, sh, 17, 8, 8), U(sw, sh, depth, 65, 8), U(sw, sh, depth, -1, 8), U(sw, sh, depth, 8, 9), U(sw, sh, depth, 8, -1)):
                    assert send(enc, bad, b, W + 2, (W + 2) // 2) == _lib.EINVAL, bad
                for k in range(3):
                    bad = U(sw, sh, depth, 8, 8)
                    bad.reserved[k] = 1
                    assert send(enc, bad, p) == _lib.EINVAL
                assert send(enc, good, p, pitch_y=sw - 1) == _lib.EINVAL and send(enc, good, p, pitch_c=sw // 2 - 1) == _lib.EINVAL
                assert send(enc, good, p, flags=4) == _lib.EINVAL
                for k in range(3):
                    assert send(enc, good, [None if j == k else p[j] for j in range(3)]) == _lib.EINVAL
            enc.send_upscaled(sw, sh, *src)
        stream = drain(enc)
        assert send(enc, good, [q.ctypes.data for q in clip(size, depth)[0]]) == _lib.ESTATE
    assert stream == reference_stream(size, depth)
    # one band of a picture coded as two slices (100x96, CTU rows 2 + 1): its session takes no upscaled source
    cfg = cfg_of(depth, W, 64)
    cfg.pic_height, cfg.slice_count, cfg.slice_index = 96, 2, 0
    cfg.slice_ctu_rows[0], cfg.slice_ctu_rows[1] = 2, 1
    cfg.rate_share_q16 = 43691
    y, u, v = clip((50, 32), depth)[0]
    full = clip((W, 64), depth)[0]
    with Encoder(cfg, device=0) as enc:
        assert send(enc, U(50, 32, depth, 8, 8), [y.ctypes.data, u.ctypes.data, v.ctypes.data], 50, 25) == _lib.EINVAL
        for k in range(N):
            enc.send(*full)
        assert len(drain(enc)) > 100


# ------------------------------------------------------------------------------------------------ 4. encode_file
def test_encode_file_with_upscale_decodes_to_the_session_reconstruction(lib, tmp_path, monkeypatch):
    from hevc_amd import encoder, mp4, probe, yuvio
    from oracle import oracle as O
    sw, sh, w, h, n = 48, 40, 96, 80, 6
    frames = [util.planes(util.synth_frame(sh, sw, seed=5, shift=(4 * i, 2 * i)), 8) for i in range(n)]
    src = tmp_path / "master.y4m"
    yuvio.write_y4m(src, frames, sw, sh, fps=30)
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
                self.size = self.coded_size()
            super().close()

    monkeypatch.setattr(encoder, "Encoder", Keeping)
    info = probe.VideoInfo(sw, sh, 30.0, "bt709", "bt709", "bt709", "yuv420p", "", "", 0, False, "eng", n, n / 30.0)
    out = tmp_path / "deliverable.mp4"
    assert encoder.encode_file(src, out, info, total_frames=n, device=0, upscale=(w, h)) == 0
    (enc,) = seen
    assert enc.size == (w, h) and (enc.cfg.width, enc.cfg.height) == (w, h)
    dec, _ = O.decode(enc.stream)
    assert len(dec) == n and all(d.same(O.Frame(*r)) for d, r in zip(dec, enc.recs))
    # and the pictures it coded are the model's: a session of the same configuration fed the model's output puts out the same bytes
    with RealEncoder(type(enc.cfg).from_buffer_copy(bytes(enc.cfg)), device=0) as ref:
        want = b""
        for i, f in enumerate(frames):
            y, u, v = R.upscale(*f, 8, w, h, 8, 8, 8)
            ref.send(y[:h, :w], u[:h // 2, :w // 2], v[:h // 2, :w // 2], pts=i)
            want += b"".join(d for d, _, _ in ref.packets())
        ref.flush()
        want += b"".join(d for d, _, _ in ref.packets())
    assert len(want) > 200 and enc.stream == want
    data = out.read_bytes()
    start, end = 0, len(data)
    for name in ("moov", "trak", "tkhd"):
        _, start, end = [b for b in mp4.parse_boxes(data, start, end) if b[0] == name][0]
    assert (int.from_bytes(data[end - 8:end - 4], "big") >> 16, int.from_bytes(data[end - 4:end], "big") >> 16) == (w, h)      # the track has the target size
    start, end = 0, len(data)
    for name in ("moov", "trak", "mdia", "minf", "stbl", "stsz"):
        _, start, end = [b for b in mp4.parse_boxes(data, start, end) if b[0] == name][0]
    assert int.from_bytes(data[start + 8:start + 12], "big") == n
