"""GPU (-m gpu): Y'CbCr sources and target sizes of the learned super-resolution on an MI355X.  1. k_sr_from_yuv alone (mihevc_k_sr_from_yuv)
bit for bit against the numpy model over the parametrisation of the stepped test; 2. the direct route: the stream of send_sr_yuv is byte for byte that of a
session fed, through send_sr, the model's 16-bit R'G'B'; 3. the resized route: the streams of send_sr_yuv and send_sr_fit into a smaller session are byte for
byte that of a plain session fed, through send_scaled at 10 bit, what mihevc_k_convert_rgb makes of mihevc_k_sr_network's half planes, a chain of existing stage
entries that the numpy models of both stages cover; every stream decodes to the session's reconstruction; 4. host planes, asynchronous host planes and device
planes (one child process) give one stream; 5. every refusal, and the session goes on; 6. a session that alternates two source sizes; 7. encode_file with a
yuv420p container and a target over a stand-in ffmpeg pipe."""
import ctypes as C
import functools
import hashlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import ingest_rgb_ref as RGB
from tests import scale_ref
from tests import sr_common as S
from tests import sr_yuv_common as Q

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("case", Q.CASES, ids=Q.case_id)
def test_stage_is_the_model(lib, case):
    Q.check_case(lib, "mihevc_k_", case, device=0)


# ------------------------------------------------------------------------------------------------ the by-hand chains
def half_planes(lib, scale, fmt, planes):
    """[3, scale H, scale W] uint16: what mihevc_k_sr_network makes of an R'G'B' source"""
    return S.network_planes(lib, S.session_model(scale), fmt, planes)


def yuv_half_planes(lib, scale, planes, B, matrix, full=False):
    return half_planes(lib, scale, *Q.rgb16_planes(planes, B, matrix, full))


def by_hand(lib, cfg, pictures, keep_recon=False):
    """the stream of a plain session fed the network's half planes of every picture: through send_rgb when they have the session's size, else through
    send_scaled (bit depth 10) after mihevc_k_convert_rgb (10 bit, the session's matrix and range).  Also the planes send_scaled was fed"""
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    fed = []
    with Encoder(cfg, device=0, keep_recon=keep_recon) as enc:
        for half in pictures:
            _, h, w = half.shape
            if (w, h) == (cfg.width, cfg.height):
                enc.send_rgb(_lib.RgbFormat(*S.HALF_PLANES), *[np.ascontiguousarray(p).view(np.float16) for p in half])
            else:
                fed.append(Q.intermediate_planes(lib, half, cfg.matrix, bool(cfg.full_range)))
                enc.send_scaled(w, h, *fed[-1], bit_depth=10)
        return Q.drain(enc), fed


def decodes_to_recon(stream, recs):
    from oracle import oracle as O
    dec, _ = O.decode(stream)
    return len(dec) == len(recs) and all(d.same(O.Frame(*r)) for d, r in zip(dec, recs))


# ------------------------------------------------------------------------------------------------ 2. the direct route
@pytest.mark.parametrize("scale,depth,src_matrix", [(4, 8, 1), (4, 8, 6), (2, 10, 9)], ids=["x4-8bit-m1", "x4-8bit-m6-into-m1", "x2-10bit-m9-into-m1"])
def test_direct_route_equals_the_session_fed_the_models_rgb(lib, scale, depth, src_matrix):
    from hevc_amd.encoder import Encoder
    sw, sh = S.SESSION_W // scale, S.SESSION_H // scale
    clip = Q.yuv_clip(sw, sh, depth)
    with Encoder(Q.session_cfg(depth), device=0, keep_recon=True) as enc:
        enc.set_sr_model(S.session_model(scale))
        for planes in clip:
            enc.send_sr_yuv(sw, sh, *planes, bit_depth=depth, matrix=src_matrix)
        got = Q.drain(enc)
        recs = [enc.recon(i) for i in range(len(clip))]
    with Encoder(Q.session_cfg(depth), device=0) as enc:
        enc.set_sr_model(S.session_model(scale))
        for planes in clip:
            fmt, rgb = Q.rgb16_planes(planes, depth, src_matrix, False)
            enc.send_sr(fmt, sw, sh, *rgb)
        want = Q.drain(enc)
    assert len(want) > 400 and got == want
    assert decodes_to_recon(got, recs)
    if src_matrix == 6:          # the source's matrix matters: the same samples read as BT.709 are another picture
        with Encoder(Q.session_cfg(depth), device=0) as enc:
            enc.set_sr_model(S.session_model(scale))
            for planes in clip:
                enc.send_sr_yuv(sw, sh, *planes, bit_depth=depth, matrix=1)
            assert Q.drain(enc) != want


# ------------------------------------------------------------------------------------------------ 3. the resized route
# (source, scale, session): 48x32 x4 = 192x128 into 108x72, the 480 -> 1080 ratio, even and no multiple of 8; 64x36 x2 = 128x72 into 96x54, the 720 -> 1080 ratio
RESIZED = [((48, 32), 4, (108, 72)), ((64, 36), 2, (96, 54))]


@functools.lru_cache(maxsize=None)
def rgb_clip(sw, sh):
    """gbrp pictures: the Y'CbCr clip's luma, mirrored two ways"""
    return [[y, np.ascontiguousarray(y[::-1]), np.ascontiguousarray(y[:, ::-1])] for y, _, _ in Q.yuv_clip(sw, sh, 8)]


@pytest.mark.parametrize("entry", ["yuv", "fit"])
@pytest.mark.parametrize("geo", RESIZED, ids=["48x32-x4-to-108x72", "64x36-x2-to-96x54"])
@pytest.mark.parametrize("depth", [8, 10])
def test_resized_route_equals_the_chain_of_stage_entries(lib, geo, entry, depth):
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    from tests.test_gpu_scale import k_scale
    (sw, sh), scale, (w, h) = geo
    cfg = Q.session_cfg(depth, w, h)
    gbrp = _lib.rgb_format_for("gbrp")
    clip = Q.yuv_clip(sw, sh, 8) if entry == "yuv" else rgb_clip(sw, sh)
    with Encoder(Q.session_cfg(depth, w, h), device=0, keep_recon=True) as enc:
        enc.set_sr_model(S.session_model(scale))
        for planes in clip:
            if entry == "yuv":
                enc.send_sr_yuv(sw, sh, *planes, bit_depth=8, matrix=6)
            else:
                enc.send_sr_fit(gbrp, sw, sh, *planes)
        got = Q.drain(enc)
        recs = [enc.recon(i) for i in range(len(clip))]
    halves = [yuv_half_planes(lib, scale, p, 8, 6) if entry == "yuv" else half_planes(lib, scale, gbrp, p) for p in clip]
    want, fed = by_hand(lib, cfg, halves)
    assert len(want) > 300 and got == want
    assert decodes_to_recon(got, recs)
    # the numpy models cover the route: ingest_rgb_ref makes the planes send_scaled was fed, and scale_ref makes of them the picture the scaler hands the session
    half_fmt = RGB.Format(0, 0, 1, 2, 1, 0)
    for half, mid in zip(halves[:2], fed[:2]):
        model_mid = RGB.convert(half_fmt, [np.ascontiguousarray(p).view(np.float16) for p in half], cfg.matrix, bool(cfg.full_range), 10)
        nh, nw = half.shape[1:]
        assert all(np.array_equal(m[:r, :c], d) for m, d, (r, c) in zip(model_mid, mid, ((nh, nw), (nh // 2, nw // 2), (nh // 2, nw // 2))))
        assert all(np.array_equal(a, b) for a, b in zip(scale_ref.scale(*mid, 10, w, h, depth), k_scale(lib, mid, 10, w, h, depth)))


# ------------------------------------------------------------------------------------------------ 4. where the source lies
@pytest.fixture(scope="module")
def device_streams():
    """SHA-256 of the streams of sessions fed device planes, from ONE child process in which torch is initialised before the library"""
    p = subprocess.run([sys.executable, "-s", "-m", "tests.sr_yuv_device_child"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    return json.loads(p.stdout[p.stdout.index("{"):])


@pytest.mark.parametrize("name,size", [("direct", (192, 128)), ("resized", (108, 72))])
def test_host_async_and_device_planes_give_one_stream(lib, device_streams, name, size):
    from hevc_amd.encoder import Encoder
    sums = {}
    for route in ("sync", "async"):
        keep = []
        with Encoder(Q.session_cfg(8, *size), device=0) as enc:
            enc.set_sr_model(S.session_model(4))
            for planes in Q.yuv_clip(48, 32, 8):
                keep.append(planes)
                enc.send_sr_yuv(48, 32, *planes, bit_depth=8, matrix=6, asynchronous=route == "async")
            sums[route] = hashlib.sha256(Q.drain(enc)).hexdigest()
    assert sums["sync"] == sums["async"] == device_streams[f"yuv-{name}"]
    if name == "resized":
        with Encoder(Q.session_cfg(8, *size), device=0) as enc:
            enc.set_sr_model(S.session_model(4))
            for planes in S.session_clip(4, 8):
                enc.send_sr_fit(S.session_format(8), 48, 32, *planes)
            assert hashlib.sha256(Q.drain(enc)).hexdigest() == device_streams["fit-resized"]


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_session_usable(lib):
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    clip = Q.yuv_clip(48, 32, 8)
    model = S.session_model(4)
    big = [np.zeros((400, 400), np.uint8)] * 3

    def send(enc, src, planes, py=None, pc=None, flags=0):
        p = [None if q is None else q.ctypes.data for q in planes]
        w = src.width if src is not None else 48
        return lib.mihevc_send_frame_sr_yuv(enc._s, None if src is None else C.byref(src), *p, w if py is None else py, w // 2 if pc is None else pc, 99, flags)

    def fit(enc, w, h, planes, pitch):
        return lib.mihevc_send_frame_sr_fit(enc._s, C.byref(S.session_format(8)), w, h, *[q.ctypes.data for q in planes], pitch, 99, 0)

    ok = _lib.SrYuv(48, 32, 8, 6, 0)
    for size in ((192, 128), (108, 72)):
        with Encoder(Q.session_cfg(8, *size), device=0) as enc:
            assert send(enc, ok, clip[0]) == _lib.EINVAL                                     # no model set
            for i, planes in enumerate(clip):
                if i == 0:
                    enc.set_sr_model(model)
                if i == 2:
                    assert send(enc, None, planes) == _lib.EINVAL
                    assert send(enc, ok, [planes[0], None, planes[2]]) == _lib.EINVAL
                    for bad in (_lib.SrYuv(48, 32, 9, 6, 0), _lib.SrYuv(48, 32, 16, 6, 0), _lib.SrYuv(48, 32, 8, 2, 0), _lib.SrYuv(48, 32, 8, 0, 0),
                                _lib.SrYuv(48, 32, 8, 6, 2)):
                        assert send(enc, bad, planes) == _lib.EINVAL, bad
                    r = _lib.SrYuv(48, 32, 8, 6, 0)
                    r.reserved[2] = 1
                    assert send(enc, r, planes) == _lib.EINVAL
                    for sw, sh in ((47, 32), (48, 31), (2, 32), (48, 2)):                       # odd sides, sides below 4
                        assert send(enc, _lib.SrYuv(sw, sh, 8, 6, 0), big, 400, 400) == _lib.EINVAL, (sw, sh)
                    assert send(enc, ok, planes, py=47) == _lib.EINVAL and send(enc, ok, planes, pc=23) == _lib.EINVAL
                    assert send(enc, ok, planes, flags=4) == _lib.EINVAL
                    # the geometry rule: a session larger than the network's output (24x16 x 4 = 96x64), a 4.5 : 1 reduction (into 108x72 a 122x82 source, which is
                    # 488x328; into 192x128 a 206x138 source, 4.3 : 1), through both entries
                    assert send(enc, _lib.SrYuv(24, 16, 8, 6, 0), big, 400, 400) == _lib.EINVAL
                    assert send(enc, _lib.SrYuv(size[0] + 14, size[1] + 10, 8, 6, 0), big, 400, 400) == _lib.EINVAL
                    assert fit(enc, 24, 16, big, 400) == _lib.EINVAL and fit(enc, size[0] + 14, size[1] + 10, big, 400) == _lib.EINVAL
                    enc.set_sr_model(None)                                                   # dropped: refused; set again: goes on
                    assert send(enc, ok, planes) == _lib.EINVAL
                    enc.set_sr_model(model)
                enc.send_sr_yuv(48, 32, *planes, bit_depth=8, matrix=6)
            stream = Q.drain(enc)
            assert send(enc, ok, clip[0]) == _lib.ESTATE and fit(enc, 48, 32, S.session_clip(4, 8)[0], 48) == _lib.ESTATE
        with Encoder(Q.session_cfg(8, *size), device=0) as enc:
            enc.set_sr_model(model)
            for planes in clip:
                enc.send_sr_yuv(48, 32, *planes, bit_depth=8, matrix=6)
            assert stream == Q.drain(enc) and len(stream) > 300
    # a cfg.matrix the conversion does not know, and a band of a picture coded as two slices
    cfg = Q.session_cfg(8, matrix=2)
    with Encoder(cfg, device=0) as enc:
        enc.set_sr_model(model)
        assert send(enc, ok, clip[0]) == _lib.EINVAL
    cfg = Q.session_cfg(8)
    cfg.height, cfg.pic_height, cfg.slice_count, cfg.slice_index = 64, 128, 2, 0
    cfg.slice_ctu_rows[0], cfg.slice_ctu_rows[1] = 2, 2
    cfg.rate_share_q16 = 32768
    with Encoder(cfg, device=0) as enc:
        assert send(enc, _lib.SrYuv(48, 16, 8, 6, 0), clip[0]) == _lib.EINVAL


def test_sr_entry_still_wants_the_exact_size(lib):
    """mihevc_send_frame_sr keeps its rule: a source the fit entry takes into a smaller session is a size mismatch there"""
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    planes = S.session_clip(4, 8)[0]
    with Encoder(Q.session_cfg(8, 108, 72), device=0) as enc:
        enc.set_sr_model(S.session_model(4))
        p = [q.ctypes.data for q in planes]
        assert lib.mihevc_send_frame_sr(enc._s, C.byref(S.session_format(8)), 48, 32, *p, 48, 0, 0) == _lib.EINVAL
        assert lib.mihevc_send_frame_sr_fit(enc._s, C.byref(S.session_format(8)), 48, 32, *p, 48, 0, 0) == 0


# ------------------------------------------------------------------------------------------------ 6. mixed sizes
def test_a_session_that_alternates_two_source_sizes(lib):
    """a 96x64 session and a x4 model: 24x16 sources take the direct route, 48x32 sources the resized one (192x128, 2 : 1); alternating them re-allocates the
    arena and the intermediate picture each time, two frames each way, against the by-hand chain"""
    from hevc_amd.encoder import Encoder
    cfg = Q.session_cfg(8, 96, 64)
    small, large = Q.yuv_clip(24, 16, 8), Q.yuv_clip(48, 32, 8)
    order = [small[0], large[1], small[2], large[3]]
    with Encoder(Q.session_cfg(8, 96, 64), device=0, keep_recon=True) as enc:
        enc.set_sr_model(S.session_model(4))
        for planes in order:
            h, w = planes[0].shape
            enc.send_sr_yuv(w, h, *planes, bit_depth=8, matrix=6, asynchronous=True)
        got = Q.drain(enc)
        recs = [enc.recon(i) for i in range(4)]
    want, fed = by_hand(lib, cfg, [yuv_half_planes(lib, 4, p, 8, 6) for p in order])
    assert len(fed) == 2 and len(want) > 200 and got == want
    assert decodes_to_recon(got, recs)


# ------------------------------------------------------------------------------------------------ 7. encode_file
def test_encode_file_with_a_yuv_container_and_a_target(lib, tmp_path, monkeypatch):
    """a stand-in ffmpeg that answers the rawvideo request with frames of zeros: the clip is asked for as yuv420p at its own size, the session, its level and
    the MP4 track open at the target, every picture goes through send_sr_yuv with BT.601 (the probe knows no matrix and the source has fewer than 720 lines),
    and the stream is that of a session of the same configuration fed the same pictures by hand"""
    from hevc_amd import encoder, mp4, probe
    from hevc_amd.transcoder import calculate_apple_hevc_level
    from tests.test_host_robustness import FAKE_FFMPEG
    sw, sh, n, target = 48, 32, 4, (108, 72)
    b = tmp_path / "bin"
    b.mkdir()
    (b / "ffmpeg").write_text(FAKE_FFMPEG)
    (b / "ffmpeg").chmod(0o755)
    monkeypatch.setenv("PATH", f"{b}:/usr/bin:/bin")
    monkeypatch.setenv("FAKE_LOG", str(tmp_path / "ffmpeg.log"))
    monkeypatch.setenv("FAKE_FRAMES", str(n))
    monkeypatch.setenv("FAKE_FB", str(sw * sh * 3 // 2))
    seen, RealEncoder = [], encoder.Encoder

    class Keeping(RealEncoder):
        """the session of encode_file, keeping what it put out"""
        def __init__(self, cfg, device=0):
            super().__init__(cfg, device=device)
            self.stream = b""
            seen.append(self)

        def packets_dts(self):
            for data, pts, key, dts in super().packets_dts():
                self.stream += data
                yield data, pts, key, dts

    monkeypatch.setattr(encoder, "Encoder", Keeping)
    info = probe.VideoInfo(sw, sh, 30.0, "", "", "", "yuv420p", "", "", 0, False, "eng", n, n / 30.0)
    out = tmp_path / "restored.mp4"
    model = S.session_model(4)
    assert encoder.encode_file(tmp_path / "rip.mkv", out, info, total_frames=n, device=0, sr_model=model, sr_target=target) == 0
    argv = (tmp_path / "ffmpeg.log").read_text().split("\n")[0].split()
    assert argv[argv.index("-pix_fmt") + 1] == "yuv420p" and not {"-s", "-vf", "-filter:v"} & set(argv)
    (enc,) = seen
    assert (enc.cfg.width, enc.cfg.height) == target
    big = probe.VideoInfo(*target, 30.0, "", "", "", "yuv420p", "", "", 0, False, "eng", n, n / 30.0)
    assert enc.cfg.level_idc == int(round(float(calculate_apple_hevc_level(big)[0]) * 30))
    zeros = [np.zeros((sh, sw), np.uint8), np.zeros((sh // 2, sw // 2), np.uint8), np.zeros((sh // 2, sw // 2), np.uint8)]
    with RealEncoder(type(enc.cfg).from_buffer_copy(bytes(enc.cfg)), device=0) as ref:
        ref.set_sr_model(model)
        want = b""
        for i in range(n):
            ref.send_sr_yuv(sw, sh, *zeros, bit_depth=8, matrix=6, pts=i)
            want += b"".join(d for d, _, _ in ref.packets())
        ref.flush()
        want += b"".join(d for d, _, _ in ref.packets())
    assert len(want) > 100 and enc.stream == want
    data = out.read_bytes()
    start, end = 0, len(data)
    for name in ("moov", "trak", "tkhd"):
        _, start, end = [x for x in mp4.parse_boxes(data, start, end) if x[0] == name][0]
    assert (int.from_bytes(data[end - 8:end - 4], "big") >> 16, int.from_bytes(data[end - 4:end], "big") >> 16) == target
