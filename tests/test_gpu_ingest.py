"""GPU (-m gpu): source conversion on an MI355X.  The kernel alone (mihevc_k_convert_source) against the numpy model of tests/ingest_ref.py, bit for bit, for every
layout and depth; sessions fed 4:2:2 / semi-planar / 4:4:4 sources through mihevc_send_frame_fmt (synchronous, asynchronous, device planes) give byte for byte
the stream of a session fed the model's 4:2:0 output through mihevc_send_frame; errors leave the session usable; encode_file on a 4:2:2 10-bit y4m."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ingest_ref as R
from tests import util
from tests.ingest_common import H, N, W, alignment_class, base_cfg, device_planes, drain, same_planes, view_of_class
from tests.test_ingest_cpu import COMBOS, combo_id, src_format

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def k_convert(lib, f, src, w, h, depth, pitch=None):
    pw, ph = R.coded(w), R.coded(h)
    out = [np.full(s, 0x77, R.out_dtype(depth)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    pitch = pitch or (src[0].shape[1], src[1].shape[1])
    rc = lib.mihevc_k_convert_source(0, C.byref(src_format(f)), *[None if p is None else p.ctypes.data for p in src], w, h, pitch[0], pitch[1], depth,
                                     *[p.ctypes.data for p in out])
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("f", COMBOS, ids=combo_id)
def test_stage_equals_model(lib, f, depth):
    for w, h in ((136, 72), (70, 38)):
        src = R.random_source(f, w, h, w + h + depth)
        diff = same_planes(k_convert(lib, f, src, w, h, depth), R.convert(f, *src, depth))
        assert not diff, (w, h, diff)


@pytest.mark.parametrize("name,depth", [("yuv422p10le", 10), ("p010le", 10), ("yuv444p", 8)])
def test_stage_equals_model_at_1080p(lib, name, depth):
    f = R.FORMATS[name]
    src = R.random_source(f, 1920, 1080, 7)
    diff = same_planes(k_convert(lib, f, src, 1920, 1080, depth), R.convert(f, *src, depth))
    assert not diff, diff


@pytest.mark.parametrize("cls", [1, 4, 8])
@pytest.mark.parametrize("f,depth", [(R.Format(444, 0, 8, 0), 8), (R.Format(444, 1, 16, 1), 10)], ids=["u8", "u16"])
def test_stage_with_misaligned_planes(lib, f, depth, cls):
    """the planes' addresses and pitches allow chunks of `cls` bytes and no wider: the element-wise (1), 4-byte and 8-byte paths on the device"""
    w, h = 70, 38
    src = R.random_source(f, w, h, 9)
    views = [None if p is None else view_of_class(p, cls) for p in src]
    assert all(alignment_class(v.ctypes.data) == alignment_class(v.strides[0]) == cls for v in views if v is not None)
    if cls == 1:
        assert views[0].ctypes.data % 16 and (views[1].strides[0] // views[1].itemsize) % 2
    pitches = (views[0].strides[0] // views[0].itemsize, views[1].strides[0] // views[1].itemsize)
    if not f.semi_planar:
        assert views[2].strides == views[1].strides
    diff = same_planes(k_convert(lib, f, views, w, h, depth, pitches), R.convert(f, *src, depth))
    assert not diff, diff


# ------------------------------------------------------------------------------------------------ 2. sessions
SESSION_FORMATS = {"yuv422p10le": 10, "nv12": 8, "yuv444p12le": 10}


@functools.lru_cache(maxsize=None)
def clip(name):
    """N pictures of a translating scene in the layout of ffmpeg format `name`"""
    f = R.FORMATS[name]
    shapes = R.plane_shapes(f, W, H)
    ch, cw = shapes[1][0], shapes[1][1] // (2 if f.semi_planar else 1)
    up = (f.bit_depth - 8) + (16 - f.bit_depth if f.msb_aligned else 0)
    out = []
    for i in range(N):
        big = util.synth_frame(2 * H, 2 * W, seed=3, shift=(2 * i, i)).y.astype(np.int64)
        y, cb, cr = big[:H, :W], big[H:H + ch, :cw], big[H:H + ch, W:W + cw]
        if f.semi_planar:
            uv = np.empty((ch, 2 * cw), np.int64)
            uv[:, 0::2], uv[:, 1::2] = cb, cr
            planes = [y, uv, None]
        else:
            planes = [y, cb, cr]
        out.append([None if p is None else np.ascontiguousarray((p << up).astype(R.src_dtype(f))) for p in planes])
    return out


@functools.lru_cache(maxsize=None)
def reference_stream(name):
    """the stream (and reconstructions) of a session fed the MODEL's 4:2:0 pictures, display size, through mihevc_send_frame"""
    from hevc_amd.encoder import Encoder
    f, depth = R.FORMATS[name], SESSION_FORMATS[name]
    with Encoder(base_cfg(depth), device=0, keep_recon=True) as enc:
        for src in clip(name):
            y, u, v = R.convert(f, *src, depth)
            enc.send(y[:H, :W], u[:H // 2, :W // 2], v[:H // 2, :W // 2])
        return drain(enc, keep_recon=True)


@pytest.mark.parametrize("route", ["sync", "async", "device"])
@pytest.mark.parametrize("name", list(SESSION_FORMATS))
def test_session_stream_equals_the_model_fed_session(lib, name, route):
    from hevc_amd.encoder import Encoder
    f, depth = R.FORMATS[name], SESSION_FORMATS[name]
    want, _ = reference_stream(name)
    keep = []
    with Encoder(base_cfg(depth), device=0) as enc:
        assert enc.coded_size() == (104, 72)
        for src in clip(name):
            if route == "device":
                src = device_planes(src)
                keep.append(src)
            elif route == "async":
                keep.append(src)
            enc.send_fmt(src_format(f), *src, asynchronous=route == "async")
        got = drain(enc)
    assert len(want) > 200 and got == want


def test_identity_format_gives_the_send_frame_stream(lib):
    from hevc_amd.encoder import Encoder
    frames = [util.planes(util.synth_frame(H, W, seed=4, shift=(2 * i, i), bit_depth=10), 10) for i in range(N)]
    streams = []
    for fmt in (None, src_format(R.Format(420, 0, 10, 0))):
        with Encoder(base_cfg(10), device=0) as enc:
            for y, u, v in frames:
                if fmt is None:
                    enc.send(y, u, v)
                else:
                    enc.send_fmt(fmt, y, u, v)
            streams.append(drain(enc))
    assert streams[0] and streams[0] == streams[1]


@pytest.mark.parametrize("name,depth", [("yuv420p", 8), ("yuv422p", 8)])
def test_device_planes_are_free_after_sync_uploads(lib, name, depth):
    """device planes at a size that already is the coded size (the plain device route would code straight from them), one set of tensors reused for every picture:
    overwritten after sync_uploads() and before the chunk fills.  The stream must be that of a session fed the same pictures from host planes, for the identity
    format as for a converted one"""
    import torch
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    f, w, h, n = R.FORMATS[name], 128, 64, 5

    def cfg():
        c = _lib.default_config()
        c.width, c.height, c.bit_depth, c.keyint, c.min_keyint, c.scenecut, c.qp, c.me_range, c.gops_in_flight, c.level_idc = w, h, depth, 3, 2, 0, 28, 12, 1, 93
        return c
    ch, cw = R.plane_shapes(f, w, h)[1]
    pics = []
    for i in range(n):
        big = util.synth_frame(2 * h, 2 * w, seed=6, shift=(2 * i, i)).y.astype(np.uint8)
        pics.append([np.ascontiguousarray(p) for p in (big[:h, :w], big[h:h + ch, :cw], big[h:h + ch, w:w + cw])])
    streams = []
    for device in (False, True):
        with Encoder(cfg(), device=0) as enc:
            assert enc.coded_size() == (w, h)
            slots = [torch.zeros(p.shape, dtype=torch.uint8, device="cuda") for p in pics[0]] if device else None
            for src in pics:
                if device:
                    for t, p in zip(slots, src):
                        t.copy_(torch.from_numpy(p))
                    torch.cuda.synchronize()
                    assert all(t.data_ptr() % 4 == 0 and t.stride(0) % 4 == 0 for t in slots)
                    enc.send_fmt(src_format(f), *slots)
                    enc.sync_uploads()
                    for t in slots:                       # the caller has its planes back
                        t.fill_(0x55)
                    torch.cuda.synchronize()
                else:
                    enc.send_fmt(src_format(f), *src)
            enc.flush()
            streams.append(b"".join(d for d, _, _ in enc.packets()))
    assert len(streams[0]) > 200 and streams[0] == streams[1]


def test_converted_stream_decodes_to_the_session_reconstruction(lib):
    from hevc_amd.encoder import Encoder
    from oracle import oracle as O
    name = "yuv422p10le"
    f, depth = R.FORMATS[name], SESSION_FORMATS[name]
    with Encoder(base_cfg(depth), device=0, keep_recon=True) as enc:
        for src in clip(name):
            enc.send_fmt(src_format(f), *src)
        stream, recs = drain(enc, keep_recon=True)
    assert stream == reference_stream(name)[0]
    dec, _ = O.decode(stream)
    assert len(dec) == N and all(d.same(O.Frame(*r)) for d, r in zip(dec, recs))


# ------------------------------------------------------------------------------------------------ 3. errors
def test_bad_calls_leave_the_session_usable(lib):
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    name = "yuv422p10le"
    f = R.FORMATS[name]
    good = src_format(f)
    with Encoder(base_cfg(10), device=0) as enc:
        for i, src in enumerate(clip(name)):
            if i == 2:
                y, u, v = (p.ctypes.data for p in src)
                bad = src_format(f)
                bad.chroma = 411
                assert lib.mihevc_send_frame_fmt(enc._s, C.byref(bad), y, u, v, W, W // 2, 99, 0) == _lib.EINVAL
                bad = src_format(f)
                bad.reserved[2] = 1
                assert lib.mihevc_send_frame_fmt(enc._s, C.byref(bad), y, u, v, W, W // 2, 99, 0) == _lib.EINVAL
                assert lib.mihevc_send_frame_fmt(enc._s, None, y, u, v, W, W // 2, 99, 0) == _lib.EINVAL
                assert lib.mihevc_send_frame_fmt(enc._s, C.byref(good), y, u, v, W, W // 2, 99, 4) == _lib.EINVAL          # an unknown flag
                assert lib.mihevc_send_frame_fmt(enc._s, C.byref(good), y, u, v, W - 1, W // 2, 99, 0) == _lib.EINVAL      # pitches smaller than the planes
                assert lib.mihevc_send_frame_fmt(enc._s, C.byref(good), y, u, v, W, W // 2 - 1, 99, 0) == _lib.EINVAL
                assert lib.mihevc_send_frame_fmt(enc._s, C.byref(good), y, u, None, W, W // 2, 99, 0) == _lib.EINVAL
            enc.send_fmt(good, *src)
        stream = drain(enc)
        y, u, v = (p.ctypes.data for p in clip(name)[0])
        assert lib.mihevc_send_frame_fmt(enc._s, C.byref(good), y, u, v, W, W // 2, N, 0) == _lib.ESTATE
    assert stream == reference_stream(name)[0]


# ------------------------------------------------------------------------------------------------ 4. encode_file
def test_encode_file_on_a_422_ten_bit_y4m(lib, tmp_path):
    from hevc_amd import encoder, mp4, probe, yuvio
    w, h, n = 96, 80, 6
    f = R.FORMATS["yuv422p10le"]
    frames = []
    for i in range(n):
        big = util.synth_frame(2 * h, 2 * w, seed=5, shift=(2 * i, i)).y.astype(np.uint16) << 2
        frames.append((big[:h, :w], big[h:2 * h, :w // 2], big[h:2 * h, w:w + w // 2]))
    src = tmp_path / "mezz.y4m"
    yuvio.write_y4m(src, frames, w, h, fps=30, bit_depth=10, chroma=422, src_depth=10)
    assert yuvio.open_clip(src).src_format == src_format(f)
    info = probe.VideoInfo(w, h, 30.0, "bt709", "bt709", "bt709", "yuv422p10le", "", "", 0, False, "eng", n, n / 30.0)
    out = tmp_path / "mezz.mp4"
    assert encoder.encode_file(src, out, info, total_frames=n, device=0) == 0
    data = out.read_bytes()
    start, end = 0, len(data)
    for name in ("moov", "trak", "mdia", "minf", "stbl", "stsz"):
        _, start, end = [b for b in mp4.parse_boxes(data, start, end) if b[0] == name][0]
    assert int.from_bytes(data[start + 8:start + 12], "big") == n
