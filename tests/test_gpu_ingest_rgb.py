"""GPU (-m gpu): RGB source conversion on an MI355X.  The kernel alone (mihevc_k_convert_rgb) against the numpy model of tests/ingest_rgb_ref.py, bit for bit, for
every layout, component order, sample type and depth; sessions fed bgra / gbrp12le / float32 pictures through mihevc_send_frame_rgb (synchronous, asynchronous,
device planes) give byte for byte the stream of a session fed the model's 4:2:0 output through mihevc_send_frame; errors leave the session usable;
encode_file with native_rgb over a stand-in ffmpeg pipe."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests import ingest_rgb_ref as R
from tests import util
from tests.ingest_common import H, N, W, alignment_class, base_cfg, device_planes, drain, same_planes, view_of_class
from tests.test_ingest_rgb_cpu import COMBOS, MATRICES, OUT_DEPTHS, combo_id, plane_ptrs, planar, rgb_format

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def k_convert(lib, f, src, w, h, matrix, full, depth, pitch=None):
    pw, ph = R.coded(w), R.coded(h)
    out = [np.full(s, 0x77, R.out_dtype(depth)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    rc = lib.mihevc_k_convert_rgb(0, C.byref(rgb_format(f, matrix, full)), *plane_ptrs(src), w, h, pitch or src[0].shape[1], depth, *[p.ctypes.data for p in out])
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("f", COMBOS, ids=combo_id)
def test_stage_equals_model(lib, f):
    n = COMBOS.index(f)
    for k, (depth, (w, h)) in enumerate(itertools.product(OUT_DEPTHS, ((136, 72), (70, 38)))):
        matrix, full = MATRICES[(n + k) % 4], bool((n + k) // 4 % 2)
        src = R.random_source(f, w, h, w + h + depth + n)
        diff = same_planes(k_convert(lib, f, src, w, h, matrix, full, depth), R.convert(f, src, matrix, full, depth))
        assert not diff, (w, h, depth, matrix, full, diff)


@pytest.mark.parametrize("name,depth", [("rgb24", 8), ("gbrp10le", 10), ("f16", 10)])
def test_stage_equals_model_at_1080p(lib, name, depth):
    f = planar(0, 1) if name == "f16" else R.FORMATS[name]
    src = R.random_source(f, 1920, 1080, 7)
    diff = same_planes(k_convert(lib, f, src, 1920, 1080, 1, False, depth), R.convert(f, src, 1, False, depth))
    assert not diff, diff


@pytest.mark.parametrize("cls", [1, 4, 8])
@pytest.mark.parametrize("name,depth", [("rgb24", 8), ("gbrp16le", 10)])
def test_stage_with_misaligned_planes(lib, name, depth, cls):
    """the planes' addresses and pitch allow chunks of `cls` bytes and no wider: the element-wise (1), 4-byte and 8-byte paths on the device"""
    f, (w, h) = R.FORMATS[name], (70, 38)
    src = R.random_source(f, w, h, 9)
    views = [view_of_class(p, cls) for p in src]
    pitch = views[0].strides[0] // views[0].itemsize
    assert all(alignment_class(v.ctypes.data) == alignment_class(v.strides[0]) == cls and v.strides == views[0].strides for v in views)
    if cls == 1:
        assert all(v.ctypes.data % 16 == v.itemsize for v in views) and pitch % 2
    diff = same_planes(k_convert(lib, f, views, w, h, 9, True, depth, pitch), R.convert(f, src, 9, True, depth))
    assert not diff, diff


# ------------------------------------------------------------------------------------------------ 2. sessions
# name -> (format, session depth, matrix and range of the format: 0 / None follow the session, which signals BT.709 limited)
SESSIONS = {"bgra": (R.FORMATS["bgra"], 8, 0, None), "gbrp12le": (R.FORMATS["gbrp12le"], 10, 9, True), "f32": (planar(0, 2), 10, 0, None)}


@functools.lru_cache(maxsize=None)
def clip(name, w=W, h=H):
    """N pictures of a translating scene in the layout of SESSIONS[name]: three different textures as R, G and B"""
    f = SESSIONS[name][0]
    out = []
    for i in range(N):
        big = util.synth_frame(2 * h, 2 * w, seed=3, shift=(2 * i, i)).y.astype(np.float64)
        rgb = [big[:h, :w], big[h:, :w], big[:h, w:]]
        if f.sample:
            comps = [(c / 255 * 1.1 - 0.05).astype(R.src_dtype(f)) for c in rgb]            # a little below 0 and above 1
        else:
            comps = [np.minimum(c * (((1 << f.bit_depth) - 1) / 255), (1 << f.bit_depth) - 1).astype(R.src_dtype(f)) for c in rgb]
        if f.layout == 0:
            planes = [None] * 3
            for k, c in zip((f.r, f.g, f.b), comps):
                planes[k] = np.ascontiguousarray(c)
        else:
            p = np.full((h, w, f.layout), 200, R.src_dtype(f))                              # the unused element: not zero
            for k, c in zip((f.r, f.g, f.b), comps):
                p[:, :, k] = c
            planes = [p.reshape(h, w * f.layout)]
        out.append(planes)
    return out


def model_planes(name, src, w=W, h=H):
    f, depth, matrix, full = SESSIONS[name]
    y, u, v = R.convert(f, src, matrix or 1, bool(full), depth)
    return y[:h, :w], u[:h // 2, :w // 2], v[:h // 2, :w // 2]


@functools.lru_cache(maxsize=None)
def reference_stream(name):
    """the stream (and reconstructions) of a session fed the MODEL's 4:2:0 pictures, display size, through mihevc_send_frame"""
    from hevc_amd.encoder import Encoder
    with Encoder(base_cfg(SESSIONS[name][1]), device=0, keep_recon=True) as enc:
        for src in clip(name):
            enc.send(*model_planes(name, src))
        return drain(enc, keep_recon=True)


def session_format(name):
    f, _, matrix, full = SESSIONS[name]
    return rgb_format(f, matrix, full)


@pytest.mark.parametrize("route", ["sync", "async", "device"])
@pytest.mark.parametrize("name", list(SESSIONS))
def test_session_stream_equals_the_model_fed_session(lib, name, route):
    from hevc_amd.encoder import Encoder
    want, _ = reference_stream(name)
    keep = []
    with Encoder(base_cfg(SESSIONS[name][1]), device=0) as enc:
        assert enc.coded_size() == (104, 72)
        for src in clip(name):
            if route == "device":
                src = device_planes(src)
            keep.append(src)
            enc.send_rgb(session_format(name), *src, asynchronous=route == "async")
        got = drain(enc)
    assert len(want) > 200 and got == want


@pytest.mark.parametrize("where", ["host", "device"])
def test_send_rgb_tensor(lib, where):
    """one (3, H, W) float32 tensor per picture, and the same pictures as (H, W, 4) uint8 tensors, through the convenience entry"""
    import torch
    from hevc_amd.encoder import Encoder
    keep = []
    with Encoder(base_cfg(10), device=0) as enc:
        for src in clip("f32"):
            t = torch.from_numpy(np.stack(src))
            t = t.cuda() if where == "device" else t
            keep.append(t)
            enc.send_rgb_tensor(t)
        assert drain(enc) == reference_stream("f32")[0]
    f = R.Format(4, 0, 1, 2, 0, 8)
    with Encoder(base_cfg(8), device=0) as enc:
        for src in clip("bgra"):
            rgba = np.ascontiguousarray(src[0].reshape(H, W, 4)[:, :, [2, 1, 0, 3]])
            t = torch.from_numpy(rgba)
            t = t.cuda() if where == "device" else t
            keep.append(t)
            enc.send_rgb_tensor(t)
        assert drain(enc) == reference_stream("bgra")[0]
        t = torch.zeros((H, W, 3), dtype=torch.uint8)
        with pytest.raises(ValueError):
            enc.send_rgb_tensor(t.permute(2, 0, 1))             # (3, H, W) with a column stride of 3
        with pytest.raises(ValueError):
            enc.send_rgb_tensor(torch.zeros((H, 2 * W, 3), dtype=torch.uint8)[:, ::2])       # pixels not side by side
        with pytest.raises(ValueError):
            enc.send_rgb_tensor(torch.zeros((3, H, W), dtype=torch.float64))


def test_device_tensors_are_free_after_sync_uploads(lib):
    """one set of device tensors reused for every picture: overwritten after sync_uploads() and before the chunk fills.  The stream must be that of the host route"""
    import torch
    from hevc_amd.encoder import Encoder
    name = "gbrp12le"
    with Encoder(base_cfg(10), device=0) as enc:
        slots = [torch.zeros((H, W), dtype=torch.int16, device="cuda") for _ in range(3)]
        for src in clip(name):
            for t, p in zip(slots, src):
                t.copy_(torch.from_numpy(p.view(np.int16)))
            torch.cuda.synchronize()
            enc.send_rgb(session_format(name), *slots)
            enc.sync_uploads()
            for t in slots:                       # the caller has its planes back
                t.fill_(0x5555)
            torch.cuda.synchronize()
        assert drain(enc) == reference_stream(name)[0]


def test_converted_stream_decodes_to_the_session_reconstruction(lib):
    from hevc_amd.encoder import Encoder
    from oracle import oracle as O
    name = "bgra"
    with Encoder(base_cfg(8), device=0, keep_recon=True) as enc:
        for src in clip(name):
            enc.send_rgb(session_format(name), *src)
        stream, recs = drain(enc, keep_recon=True)
    assert stream == reference_stream(name)[0]
    dec, _ = O.decode(stream)
    assert len(dec) == N and all(d.same(O.Frame(*r)) for d, r in zip(dec, recs))


# ------------------------------------------------------------------------------------------------ 3. errors
def test_bad_calls_leave_the_session_usable(lib):
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    name = "gbrp12le"
    good = session_format(name)
    with Encoder(base_cfg(10), device=0) as enc:
        for i, src in enumerate(clip(name)):
            if i == 2:
                p = [q.ctypes.data for q in src]
                send = lambda fmt, planes=p, pitch=W, flags=0: lib.mihevc_send_frame_rgb(enc._s, None if fmt is None else C.byref(fmt), *planes, pitch, 99, flags)

                def bad(**fields):
                    fmt = session_format(name)
                    for k, v in fields.items():
                        setattr(fmt, k, v)
                    return fmt
                assert send(None) == _lib.EINVAL
                for fields in (dict(layout=2), dict(r=1), dict(g=3), dict(bit_depth=17), dict(sample=1), dict(sample=2, bit_depth=0, layout=3), dict(matrix=2),
                               dict(range=3)):
                    assert send(bad(**fields)) == _lib.EINVAL, fields
                fmt = bad()
                fmt.reserved[2] = 1
                assert send(fmt) == _lib.EINVAL
                assert send(good, flags=4) == _lib.EINVAL                                # an unknown flag
                assert send(good, pitch=W - 1) == _lib.EINVAL                            # a pitch smaller than the row
                assert send(good, planes=[p[0], p[1], None]) == _lib.EINVAL              # a plane the layout needs
                assert send(good, planes=[p[0], p[1] + 1, p[2]]) == _lib.EINVAL          # a 16-bit plane at an odd address
            enc.send_rgb(good, *src)
        stream = drain(enc)
        assert lib.mihevc_send_frame_rgb(enc._s, C.byref(good), *[q.ctypes.data for q in clip(name)[0]], W, N, 0) == _lib.ESTATE
    assert stream == reference_stream(name)[0]


def test_session_configurations_the_entry_refuses(lib):
    """decided by the session's configuration: a signalled matrix that is no Y'CbCr matrix with nothing explicit in the format, bands of a picture; an odd
    size, which the entry also checks, is refused by mihevc_open already"""
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    f = R.FORMATS["gbrp"]
    for matrix in (0, 2):
        cfg = base_cfg(8)
        cfg.matrix = matrix
        with Encoder(cfg, device=0) as enc:
            src = [np.zeros((H, W), np.uint8)] * 3
            p = [q.ctypes.data for q in src]
            assert lib.mihevc_send_frame_rgb(enc._s, C.byref(rgb_format(f)), *p, W, 0, 0) == _lib.EINVAL
            assert lib.mihevc_send_frame_rgb(enc._s, C.byref(rgb_format(f, 6)), *p, W, 0, 0) == 0          # explicit in the format: fine, and the session lives
            enc.flush()
            assert len(list(enc.packets())) == 1
    cfg = base_cfg(8)
    cfg.width = W - 1                             # an odd size does not get as far as a session
    assert lib.mihevc_open(C.byref(cfg), 0, C.byref(C.c_void_p())) == _lib.EINVAL
    cfg = _lib.default_config()
    cfg.width, cfg.height, cfg.pic_height, cfg.slice_count, cfg.slice_index, cfg.level_idc, cfg.qp = 160, 64, 96, 2, 0, 63, 28
    cfg.slice_ctu_rows[0], cfg.slice_ctu_rows[1] = 2, 1
    with Encoder(cfg, device=0) as enc:
        src = [np.zeros((64, 160), np.uint8)] * 3
        assert lib.mihevc_send_frame_rgb(enc._s, C.byref(rgb_format(f)), *[q.ctypes.data for q in src], 160, 0, 0) == _lib.EINVAL


# ------------------------------------------------------------------------------------------------ 4. encode_file
@pytest.mark.parametrize("pix,devices", [("gbrp10le", None), ("bgr0", [0, 0])], ids=["one-session", "sharded"])
def test_encode_file_native_rgb_over_the_pipe(lib, tmp_path, monkeypatch, pix, devices):
    """a stand-in ffmpeg that answers the rawvideo request with FAKE_FRAMES frames of zeros: the clip is asked for in its own RGB format and coded through
    send_rgb, by one session (three planes) and by a ShardedEncoder of two sessions (one packed plane per picture, GOP chunks round-robin)"""
    from hevc_amd import _lib, encoder, mp4, probe
    from tests.test_host_robustness import FAKE_FFMPEG
    w, h, n = 96, 80, 6
    b = tmp_path / "bin"
    b.mkdir()
    (b / "ffmpeg").write_text(FAKE_FFMPEG)
    (b / "ffmpeg").chmod(0o755)
    monkeypatch.setenv("PATH", f"{b}:/usr/bin:/bin")
    monkeypatch.setenv("FAKE_LOG", str(tmp_path / "ffmpeg.log"))
    monkeypatch.setenv("FAKE_FRAMES", str(n))
    monkeypatch.setenv("FAKE_FB", str(_lib.rgb_format_for(pix).frame_bytes(w, h)))
    info = probe.VideoInfo(w, h, 30.0, "bt709", "bt709", "gbr", pix, "", "", 0, False, "eng", n, n / 30.0)
    out = tmp_path / "screen.mp4"
    assert encoder.encode_file(tmp_path / "screen.mkv", out, info, total_frames=n, device=0, devices=devices, native_rgb=True) == 0
    argv = (tmp_path / "ffmpeg.log").read_text().split("\n")[0].split()
    assert argv[argv.index("-pix_fmt") + 1] == pix
    data = out.read_bytes()
    start, end = 0, len(data)
    for name in ("moov", "trak", "mdia", "minf", "stbl", "stsz"):
        _, start, end = [b for b in mp4.parse_boxes(data, start, end) if b[0] == name][0]
    assert int.from_bytes(data[start + 8:start + 12], "big") == n


def test_sharded_sessions_take_rgb_pictures(lib):
    """ShardedEncoder.send with an RgbFormat: three planes, and one packed plane with u and v None, give the streams of single sessions"""
    from hevc_amd.encoder import ShardedEncoder
    for name in ("gbrp12le", "bgra"):
        sh = ShardedEncoder(base_cfg(SESSIONS[name][1]), [0])
        try:
            for src in clip(name):
                sh.send(*(tuple(src) + (None, None))[:3], session_format(name))
            got = sorted(sh.finish(), key=lambda x: x[1])
        finally:
            sh.close()
        assert b"".join(d for d, _, _ in got) == reference_stream(name)[0], name


def test_send_rgb_rejects_planes_the_kernel_cannot_read(lib):
    import torch
    from hevc_amd.encoder import Encoder
    fmt = session_format("gbrp12le")
    with Encoder(base_cfg(10), device=0) as enc:
        a, b = torch.zeros((H, W), dtype=torch.int16, device="cuda"), torch.zeros((H, W + 8), dtype=torch.int16, device="cuda")
        with pytest.raises(ValueError, match="one pitch"):
            enc.send_rgb(fmt, a, a, b[:, :W])                           # the third plane's rows are 8 samples further apart
        with pytest.raises(ValueError):
            enc.send_rgb(fmt, a, a, torch.zeros((H, 2 * W), dtype=torch.int16, device="cuda")[:, ::2])      # column stride 2
        with pytest.raises(ValueError):
            enc.send_rgb(fmt, a, a)                                     # a plane short
        with pytest.raises(ValueError):
            enc.send_rgb(fmt, a, a, a.to(torch.float16))                # floats handed over as integers
        with pytest.raises(ValueError):
            enc.send_rgb(fmt, *[np.zeros((H, W), np.uint8)] * 3)        # host planes of the wrong element size
        for src in clip("gbrp12le"):                                    # and the session is as good as new
            enc.send_rgb(fmt, *src)
        assert drain(enc) == reference_stream("gbrp12le")[0]
