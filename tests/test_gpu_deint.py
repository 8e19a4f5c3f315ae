"""GPU (-m gpu): the deinterlacing source on an MI355X.  The kernel alone (mihevc_k_deinterlace) against the numpy model of tests/deint_ref.py, bit
for bit, over the sizes and combinations of the CPU tests, misaligned planes and one 1080p picture; sessions fed woven frames through mihevc_send_frame_deint
(synchronous, asynchronous, device planes) give byte for byte the stream of a session fed the model's pictures through mihevc_send_frame, in frame and field
mode and both field orders; errors leave the session usable."""
import ctypes as C
import functools
import hashlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import deint_ref as R
from tests.deint_common import COMBOS, H, KINDS, N_FRAMES, SIZES, W, cfg_of, clip, frames, model, model_pictures, plane_pointers
from tests.ingest_common import alignment_class, same_planes, view_of_class

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def k_deint(lib, P, Cc, N, depth, keep, second, pitch=None):
    h, w = Cc[0].shape
    pw, ph = R.coded(w), R.coded(h)
    out = [np.full(s, 0x77, R.dtype(depth)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    pitch = pitch or (w, w // 2)
    rc = lib.mihevc_k_deinterlace(0, plane_pointers(P), plane_pointers(Cc), plane_pointers(N), w, h, pitch[0], pitch[1], depth, keep, second, *[p.ctypes.data for p in out])
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stage_equals_model(lib, size, depth):
    for kind in KINDS:
        for keep, second in COMBOS:
            diff = same_planes(k_deint(lib, *frames(size, depth, kind), depth, keep, second), model(size, depth, kind, keep, second)[0])
            assert not diff, (kind, keep, second, diff)


@pytest.mark.parametrize("cls", [1, 4, 8])
@pytest.mark.parametrize("depth", [8, 10])
def test_stage_with_misaligned_planes(lib, depth, cls):
    """the planes' addresses and pitches allow chunks of `cls` bytes and no wider"""
    for size, (keep, second) in ((SIZES[0], (0, 1)), (SIZES[1], (1, 0))):
        views = [[view_of_class(p, cls) for p in f] for f in frames(size, depth, "noise")]
        assert all(alignment_class(v.ctypes.data) == alignment_class(v.strides[0]) == cls for f in views for v in f)
        assert len({f[0].strides for f in views}) == 1 and len({f[k].strides for f in views for k in (1, 2)}) == 1
        pitches = (views[0][0].strides[0] // views[0][0].itemsize, views[0][1].strides[0] // views[0][1].itemsize)
        diff = same_planes(k_deint(lib, *views, depth, keep, second, pitches), model(size, depth, "noise", keep, second)[0])
        assert not diff, (size, diff)


def test_stage_equals_model_at_1080p(lib):
    """tile counts and index ranges of a real picture: 1920x1080, 8 bit"""
    fr = R.noise_frames(1920, 1080, 8, 7)
    diff = same_planes(k_deint(lib, *fr, 8, 0, 1), R.deinterlace(*fr, 8, 0, 1)[0])
    assert not diff, diff


def test_stage_with_one_frame_for_all_three(lib):
    (f,) = R.woven_frames(70, 36, 8, 1)
    for keep, second in COMBOS:
        diff = same_planes(k_deint(lib, f, f, f, 8, keep, second), R.deinterlace(f, f, f, 8, keep, second)[0])
        assert not diff, diff


# ------------------------------------------------------------------------------------------------ 2. sessions
def drain(enc):
    enc.flush()
    got = list(enc.packets())
    return b"".join(d for d, _, _ in got), [p for _, p, _ in got]


@functools.lru_cache(maxsize=None)
def reference_stream(depth, tff, field_rate, n=N_FRAMES):
    """(stream, pts list) of a session fed the MODEL's pictures, display size, through mihevc_send_frame"""
    from hevc_amd.encoder import Encoder
    with Encoder(cfg_of(depth, field_rate), device=0) as enc:
        for pts, (y, u, v) in model_pictures(depth, tff, field_rate, n):
            enc.send(y, u, v, pts=pts)
        return drain(enc)


@pytest.mark.parametrize("route", ["sync", "async"])
@pytest.mark.parametrize("field_rate", [False, True], ids=["frame", "field"])
@pytest.mark.parametrize("tff", [True, False], ids=["tff", "bff"])
@pytest.mark.parametrize("depth", [8, 10])
def test_session_stream_equals_the_model_fed_session(lib, depth, tff, field_rate, route):
    from hevc_amd.encoder import Encoder
    want, want_pts = reference_stream(depth, tff, field_rate)
    with Encoder(cfg_of(depth, field_rate), device=0) as enc:
        assert enc.coded_size() == (104, 72)
        for i, src in enumerate(clip(depth, tff)):
            enc.send_deint(*src, tff=tff, field_rate=field_rate, asynchronous=route == "async")
            assert enc.stats().frames_in == i * (2 if field_rate else 1)          # pictures, and a frame's come when the next frame arrives
        got, pts = drain(enc)
        assert enc.stats().frames_in == N_FRAMES * (2 if field_rate else 1)
    assert len(want) > 200 and got == want
    assert pts == want_pts and sorted(pts) == list(range(N_FRAMES * (2 if field_rate else 1)))


@pytest.fixture(scope="module")
def device_streams():
    """SHA-256 and pts of the streams of sessions fed from torch tensors, from ONE child process in which torch is initialised before the library
    (tests/deint_device_child.py says why): what this test is about is that order"""
    p = subprocess.run([sys.executable, "-s", "-m", "tests.deint_device_child"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    return json.loads(p.stdout[p.stdout.index("{"):])


@pytest.mark.parametrize("field_rate", [False, True], ids=["frame", "field"])
@pytest.mark.parametrize("tff", [True, False], ids=["tff", "bff"])
@pytest.mark.parametrize("depth", [8, 10])
def test_session_fed_device_planes_equals_the_model_fed_session(lib, device_streams, depth, tff, field_rate):
    want, want_pts = reference_stream(depth, tff, field_rate)
    assert len(want) > 200 and device_streams[f"{depth}-{int(tff)}-{int(field_rate)}"] == [hashlib.sha256(want).hexdigest(), want_pts]


@pytest.mark.parametrize("field_rate", [False, True], ids=["frame", "field"])
def test_a_one_frame_clip(lib, field_rate):
    """P = C = N: flush produces the picture(s)"""
    from hevc_amd.encoder import Encoder
    want, want_pts = reference_stream(8, True, field_rate, 1)
    with Encoder(cfg_of(8, field_rate), device=0) as enc:
        enc.send_deint(*clip(8, True, 1)[0], tff=True, field_rate=field_rate)
        assert enc.stats().frames_in == 0
        got, pts = drain(enc)
    assert len(want) > 100 and got == want and pts == want_pts == list(range(2 if field_rate else 1))


# ------------------------------------------------------------------------------------------------ 3. errors
def test_bad_calls_leave_the_session_usable(lib):
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    depth, tff = 8, True
    good = _lib.Deint(1, 0)

    def send(enc, mode, planes, pitch_y=W, pitch_c=W // 2, flags=0):
        return lib.mihevc_send_frame_deint(enc._s, None if mode is None else C.byref(mode), *planes, pitch_y, pitch_c, 99, flags)

    with Encoder(cfg_of(depth), device=0) as enc:
        for i, src in enumerate(clip(depth, tff)):
            p = [q.ctypes.data for q in src]
            if i in (0, 2):          # before the first frame fixes the mode, and with a frame pending
                assert send(enc, None, p) == _lib.EINVAL
                for bad in (_lib.Deint(2, 0), _lib.Deint(-1, 0), _lib.Deint(1, 2), _lib.Deint(1, -1)):
                    assert send(enc, bad, p) == _lib.EINVAL, bad
                for k in range(6):
                    bad = _lib.Deint(1, 0)
                    bad.reserved[k] = 1
                    assert send(enc, bad, p) == _lib.EINVAL
                assert send(enc, good, p, pitch_y=W - 1) == _lib.EINVAL and send(enc, good, p, pitch_c=W // 2 - 1) == _lib.EINVAL
                assert send(enc, good, p, flags=4) == _lib.EINVAL
                for k in range(3):
                    assert send(enc, good, [None if j == k else q for j, q in enumerate(p)]) == _lib.EINVAL
            if i == 2:               # the mode of the first frame holds; any other entry must wait for flush
                assert send(enc, _lib.Deint(0, 0), p) == _lib.EINVAL and send(enc, _lib.Deint(1, 1), p) == _lib.EINVAL
                assert lib.mihevc_send_frame(enc._s, *p, W, W // 2, 99) == _lib.ESTATE
                assert lib.mihevc_send_frame_async(enc._s, *p, W, W // 2, 99) == _lib.ESTATE
                assert lib.mihevc_send_frame_fmt(enc._s, C.byref(_lib.SrcFormat(422, 0, 8, 0)), *p, W, W // 2, 99, 0) == _lib.ESTATE
                assert lib.mihevc_send_frame_scaled(enc._s, C.byref(_lib.ScaleSrc(W, H, 8)), *p, W, W // 2, 99, 0) == _lib.ESTATE
            enc.send_deint(*src, tff=tff)
        stream, pts = drain(enc)
        assert send(enc, good, [q.ctypes.data for q in clip(depth, tff)[0]]) == _lib.ESTATE
    assert (stream, pts) == reference_stream(depth, tff, False)
    # sizes the filter does not take: a height that is no multiple of 4; one band of a picture coded as two slices
    y, u, v = (np.zeros(s, np.uint8) for s in ((70, W), (35, W // 2), (35, W // 2)))
    cfg = cfg_of(depth)
    cfg.height = 70
    with Encoder(cfg, device=0) as enc:
        assert send(enc, good, [y.ctypes.data, u.ctypes.data, v.ctypes.data]) == _lib.EINVAL
        for k in range(3):
            enc.send(y, u, v)
        assert len(drain(enc)[0]) > 50
    cfg = cfg_of(depth)
    cfg.height = 64
    cfg.pic_height, cfg.slice_count, cfg.slice_index = 96, 2, 0
    cfg.slice_ctu_rows[0], cfg.slice_ctu_rows[1] = 2, 1
    cfg.rate_share_q16 = 43691
    with Encoder(cfg, device=0) as enc:
        assert send(enc, good, [y.ctypes.data, u.ctypes.data, v.ctypes.data]) == _lib.EINVAL
        for k in range(3):
            enc.send(y[:64], u[:32], v[:32])
        assert len(drain(enc)[0]) > 50
