"""GPU (-m gpu): the denoising source on an MI355X.  The kernel alone (mihevc_k_denoise) against the numpy model of tests/denoise_ref.py, bit for
bit, over the sizes, depths and strengths of the CPU tests, misaligned planes and one 1080p picture; sessions fed noisy frames through
mihevc_send_frame_denoise (synchronous, asynchronous, device planes) give byte for byte the stream of a session fed the model's pictures through
mihevc_send_frame; errors leave the session usable."""
import ctypes as C
import functools
import hashlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import denoise_ref as R
from tests.denoise_common import CHANGING, H, KINDS, N_FRAMES, SIZES, STRENGTHS, W, cfg_of, clip, denoise_struct, frames, model, model_pictures, plane_pointers, strength_id
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
def k_denoise(lib, P, Cc, N, depth, strength, pitch=None):
    h, w = Cc[0].shape
    pw, ph = R.coded(w), R.coded(h)
    out = [np.full(s, 0x77, R.dtype(depth)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    pitch = pitch or (w, w // 2)
    rc = lib.mihevc_k_denoise(0, C.byref(denoise_struct(strength)), plane_pointers(P), plane_pointers(Cc), plane_pointers(N), w, h, pitch[0], pitch[1], depth,
                              *[p.ctypes.data for p in out])
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stage_equals_model(lib, size, depth):
    for kind in KINDS:
        for strength in STRENGTHS:
            diff = same_planes(k_denoise(lib, *frames(size, depth, kind), depth, strength), model(size, depth, kind, strength)[0])
            assert not diff, (kind, strength, diff)


@pytest.mark.parametrize("cls", [1, 4, 8])
@pytest.mark.parametrize("depth", [8, 10])
def test_stage_with_misaligned_planes(lib, depth, cls):
    """the planes' addresses and pitches allow chunks of `cls` bytes and no wider"""
    for size, strength in ((SIZES[1], STRENGTHS[1]), (SIZES[2], STRENGTHS[3])):
        views = [[view_of_class(p, cls) for p in f] for f in frames(size, depth, "noise")]
        assert all(alignment_class(v.ctypes.data) == alignment_class(v.strides[0]) == cls for f in views for v in f)
        assert len({f[0].strides for f in views}) == 1 and len({f[k].strides for f in views for k in (1, 2)}) == 1
        pitches = (views[0][0].strides[0] // views[0][0].itemsize, views[0][1].strides[0] // views[0][1].itemsize)
        diff = same_planes(k_denoise(lib, *views, depth, strength, pitches), model(size, depth, "noise", strength)[0])
        assert not diff, (size, diff)


def test_stage_equals_model_at_1080p(lib):
    """tile counts and index ranges of a real picture: 1920x1080, 8 bit"""
    fr = R.noise_frames(1920, 1080, 8, 7)
    diff = same_planes(k_denoise(lib, *fr, 8, (40, 60, 30, 50)), R.denoise(*fr, 8, (40, 60, 30, 50))[0])
    assert not diff, diff


def test_stage_with_one_frame_for_all_three(lib):
    f = R.noisy_frames(70, 36, 8, 1, 0)[0][0]
    for strength in STRENGTHS:
        diff = same_planes(k_denoise(lib, f, f, f, 8, strength), R.denoise(f, f, f, 8, strength)[0])
        assert not diff, diff


# ------------------------------------------------------------------------------------------------ 2. sessions
def drain(enc):
    enc.flush()
    got = list(enc.packets())
    return b"".join(d for d, _, _ in got), [p for _, p, _ in got]


@functools.lru_cache(maxsize=None)
def reference_stream(depth, strength, n=N_FRAMES):
    """(stream, pts list) of a session fed the MODEL's pictures, display size, through mihevc_send_frame; strength None: the clip itself"""
    from hevc_amd.encoder import Encoder
    with Encoder(cfg_of(depth), device=0) as enc:
        if strength is None:
            for src in clip(depth, n):
                enc.send(*src)
        else:
            for pts, (y, u, v) in model_pictures(depth, strength, n):
                enc.send(y, u, v, pts=pts)
        return drain(enc)


@pytest.mark.parametrize("route", ["sync", "async"])
@pytest.mark.parametrize("strength", [2, (12, 0, 0, 16)], ids=strength_id)
@pytest.mark.parametrize("depth", [8, 10])
def test_session_stream_equals_the_model_fed_session(lib, depth, strength, route):
    from hevc_amd.encoder import Encoder
    want, want_pts = reference_stream(depth, strength)
    with Encoder(cfg_of(depth), device=0) as enc:
        assert enc.coded_size() == (104, 72)
        for i, src in enumerate(clip(depth)):
            enc.send_denoise(*src, strength=strength, asynchronous=route == "async")
            assert enc.stats().frames_in == i          # pictures, and a frame's comes when the next frame arrives
        got, pts = drain(enc)
        assert enc.stats().frames_in == N_FRAMES
    assert len(want) > 200 and got == want
    assert pts == want_pts and sorted(pts) == list(range(N_FRAMES))
    assert want != reference_stream(depth, None)[0]          # the filter did something to the clip


@pytest.fixture(scope="module")
def device_streams():
    """SHA-256 and pts of the streams of sessions fed from torch tensors, from ONE child process in which torch is initialised before the library
    (tests/denoise_device_child.py says why): what this test is about is that order"""
    p = subprocess.run([sys.executable, "-s", "-m", "tests.denoise_device_child"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    return json.loads(p.stdout[p.stdout.index("{"):])


@pytest.mark.parametrize("strength", [2, "changing"], ids=str)
@pytest.mark.parametrize("depth", [8, 10])
def test_session_fed_device_planes_equals_the_model_fed_session(lib, device_streams, depth, strength):
    want, want_pts = reference_stream(depth, strength)
    assert len(want) > 200 and device_streams[f"{depth}-{strength}"] == [hashlib.sha256(want).hexdigest(), want_pts]


@pytest.mark.parametrize("depth", [8, 10])
def test_a_one_frame_clip(lib, depth):
    """P = C = N: flush produces the picture"""
    from hevc_amd.encoder import Encoder
    want, want_pts = reference_stream(depth, 3, 1)
    with Encoder(cfg_of(depth), device=0) as enc:
        enc.send_denoise(*clip(depth, 1)[0], strength=3)
        assert enc.stats().frames_in == 0
        got, pts = drain(enc)
        assert enc.stats().frames_in == 1
    assert len(want) > 100 and got == want and pts == want_pts == [0]


@pytest.mark.parametrize("depth", [8, 10])
def test_strengths_changing_inside_a_clip(lib, depth):
    """the strengths sent with frame k apply to picture k, which is produced one call later"""
    from hevc_amd.encoder import Encoder
    want, want_pts = reference_stream(depth, "changing")
    with Encoder(cfg_of(depth), device=0) as enc:
        for src, strength in zip(clip(depth), CHANGING):
            enc.send_denoise(*src, strength=strength)
        got, pts = drain(enc)
    assert len(want) > 200 and got == want and pts == want_pts
    assert want != reference_stream(depth, 2)[0]


@pytest.mark.parametrize("depth", [8, 10])
def test_zero_strengths_give_the_stream_of_plain_send(lib, depth):
    from hevc_amd.encoder import Encoder
    want, want_pts = reference_stream(depth, None)
    with Encoder(cfg_of(depth), device=0) as enc:
        for src in clip(depth):
            enc.send_denoise(*src, strength=0)
        got, pts = drain(enc)
    assert len(want) > 200 and got == want and pts == want_pts


# ------------------------------------------------------------------------------------------------ 3. errors
def test_bad_calls_leave_the_session_usable(lib):
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    depth = 8
    good = _lib.denoise_level(2)

    def send(enc, dn, planes, pitch_y=W, pitch_c=W // 2, flags=0):
        return lib.mihevc_send_frame_denoise(enc._s, None if dn is None else C.byref(dn), *planes, pitch_y, pitch_c, 99, flags)

    with Encoder(cfg_of(depth), device=0) as enc:
        for i, src in enumerate(clip(depth)):
            p = [q.ctypes.data for q in src]
            if i in (0, 2):          # before the first frame, and with a frame pending
                assert send(enc, None, p) == _lib.EINVAL
                for k in range(4):
                    for v in (-1, 256):
                        t = [5, 7, 5, 7]
                        t[k] = v
                        assert send(enc, _lib.Denoise(*t), p) == _lib.EINVAL, t
                    bad = _lib.denoise_level(2)
                    bad.reserved[k] = 1
                    assert send(enc, bad, p) == _lib.EINVAL
                assert send(enc, good, p, pitch_y=W - 1) == _lib.EINVAL and send(enc, good, p, pitch_c=W // 2 - 1) == _lib.EINVAL
                assert send(enc, good, p, flags=4) == _lib.EINVAL
                for k in range(3):
                    assert send(enc, good, [None if j == k else q for j, q in enumerate(p)]) == _lib.EINVAL
            if i == 2:               # any other entry must wait for flush
                assert lib.mihevc_send_frame(enc._s, *p, W, W // 2, 99) == _lib.ESTATE
                assert lib.mihevc_send_frame_async(enc._s, *p, W, W // 2, 99) == _lib.ESTATE
                assert lib.mihevc_send_frame_fmt(enc._s, C.byref(_lib.SrcFormat(422, 0, 8, 0)), *p, W, W // 2, 99, 0) == _lib.ESTATE
                assert lib.mihevc_send_frame_scaled(enc._s, C.byref(_lib.ScaleSrc(W, H, 8)), *p, W, W // 2, 99, 0) == _lib.ESTATE
                assert lib.mihevc_send_frame_deint(enc._s, C.byref(_lib.Deint(1, 0)), *p, W, W // 2, 99, 0) == _lib.ESTATE
            enc.send_denoise(*src, strength=2)
        stream, pts = drain(enc)
        assert send(enc, good, [q.ctypes.data for q in clip(depth)[0]]) == _lib.ESTATE          # after flush
        assert lib.mihevc_send_frame(enc._s, *[q.ctypes.data for q in clip(depth)[0]], W, W // 2, 99) == _lib.ESTATE
    assert (stream, pts) == reference_stream(depth, 2)


def test_denoise_waits_while_a_deinterlaced_frame_is_pending(lib):
    """mihevc_send_frame_denoise returns MIHEVC_ESTATE while a deinterlaced frame is pending, and the deinterlacing session goes on as if it had not been called"""
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    outs = []
    for poke in (False, True):
        with Encoder(cfg_of(8), device=0) as enc:
            for i, src in enumerate(clip(8)):
                enc.send_deint(*src, tff=True)
                if poke and i in (0, 3):
                    p = [q.ctypes.data for q in src]
                    assert lib.mihevc_send_frame_denoise(enc._s, C.byref(_lib.denoise_level(2)), *p, W, W // 2, 99, 0) == _lib.ESTATE
            outs.append(drain(enc))
    assert len(outs[0][0]) > 200 and outs[0] == outs[1]


def test_sizes_and_sessions_the_filter_does_not_take(lib):
    """one band of a picture coded as two slices: MIHEVC_EINVAL, and the session codes on (a session has no odd size and none below 16: mihevc_k_denoise refuses
    those, tests/test_denoise_cpu.py)"""
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    good = _lib.denoise_level(2)
    y, u, v = (np.zeros(s, np.uint8) for s in ((64, W), (32, W // 2), (32, W // 2)))
    cfg = cfg_of(8)
    cfg.height = 64
    cfg.pic_height, cfg.slice_count, cfg.slice_index = 96, 2, 0
    cfg.slice_ctu_rows[0], cfg.slice_ctu_rows[1] = 2, 1
    cfg.rate_share_q16 = 43691
    with Encoder(cfg, device=0) as enc:
        assert lib.mihevc_send_frame_denoise(enc._s, C.byref(good), y.ctypes.data, u.ctypes.data, v.ctypes.data, W, W // 2, 0, 0) == _lib.EINVAL
        for k in range(3):
            enc.send(y, u, v)
        assert len(drain(enc)[0]) > 50
