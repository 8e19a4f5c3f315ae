"""GPU (-m gpu): frame-rate multiplication on an MI355X.  The kernels alone (mihevc_k_mcfi_vectors, mihevc_k_mcfi_render) against the numpy model
of tests/mcfi_ref.py, bit for bit, over the sizes, kinds, depths and factors of the CPU tests, extreme fields, misaligned planes and one 1080p pair; sessions fed
frames through mihevc_send_frame_interpolate (synchronous, asynchronous, device planes) give byte for byte the stream of a session fed the model's pictures
through mihevc_send_frame; errors leave the session usable."""
import ctypes as C
import functools
import hashlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import mcfi_ref as R
from tests.ingest_common import alignment_class, same_planes, view_of_class
from tests.mcfi_common import (FACTORS, H, KINDS, N_FRAMES, SIZES, W, cfg_of, clip, extreme_fields, frames, interpolate_struct, model_picture, model_pictures, model_vectors,
                               pan_frames, plane_pointers)

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


# ------------------------------------------------------------------------------------------------ 1. the kernels alone
def k_vectors(lib, c, n, depth, pitch=None):
    h, w = c[0].shape
    v0, v, D = np.full((R.blocks(h), R.blocks(w), 2), 99, np.int16), np.full((R.blocks(h), R.blocks(w), 2), 99, np.int16), C.c_uint64(1)
    rc = lib.mihevc_k_mcfi_vectors(0, c[0].ctypes.data, n[0].ctypes.data, w, h, pitch or w, depth, v0.ctypes.data, v.ctypes.data, C.addressof(D))
    assert rc == 0, rc
    return v0, v, D.value


def k_render(lib, c, n, depth, f, j, v, D, mode=0, thr=10, pitch=None):
    h, w = c[0].shape
    pw, ph = (w + 7) & ~7, (h + 7) & ~7
    out = [np.full(s, 0x77, R.dtype(depth)) for s in ((ph, pw), (ph // 2, pw // 2), (ph // 2, pw // 2))]
    pitch = pitch or (w, w // 2)
    rc = lib.mihevc_k_mcfi_render(0, C.byref(interpolate_struct(f, mode, thr)), j, plane_pointers(c), plane_pointers(n), None if v is None else v.ctypes.data, D, w, h,
                                  pitch[0], pitch[1], depth, *[p.ctypes.data for p in out])
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_vectors_equal_model(lib, size, depth):
    """v0, v and D, every block of every kind: the key makes every decision total, so nothing is excluded"""
    for kind in KINDS:
        v0, v, D = k_vectors(lib, *frames(size, depth, kind), depth)
        want = model_vectors(size, depth, kind)
        assert np.array_equal(v0, want[0]), (kind, "v0", int((v0 != want[0]).any(axis=2).sum()))
        assert np.array_equal(v, want[1]), (kind, "v", int((v != want[1]).any(axis=2).sum()))
        assert D == want[2], (kind, D, want[2])


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_render_equals_model(lib, size, depth):
    for kind in KINDS:
        c, n = frames(size, depth, kind)
        _, v, D = model_vectors(size, depth, kind)
        for f in FACTORS:
            for j in range(f):
                for thr in (0, 10):
                    diff = same_planes(k_render(lib, c, n, depth, f, j, v, D, 0, thr), model_picture(size, depth, kind, f, j, 0, thr))
                    assert not diff, (kind, f, j, thr, diff)
        diff = same_planes(k_render(lib, c, n, depth, 3, 2, None, 0, 1), model_picture(size, depth, kind, 3, 2, 1))
        assert not diff, (kind, "blend", diff)


@pytest.mark.parametrize("cls", [1, 4, 8])
@pytest.mark.parametrize("depth", [8, 10])
def test_render_with_extreme_fields_and_misaligned_planes(lib, depth, cls):
    """+-18 in every block and alternating signs, planes whose addresses and pitches allow chunks of `cls` bytes and no wider"""
    for size in SIZES:
        c, n = frames(size, depth, "noise")
        views = [[view_of_class(p, cls) for p in f] for f in (c, n)]
        assert all(alignment_class(v.ctypes.data) == alignment_class(v.strides[0]) == cls for f in views for v in f)
        assert len({f[0].strides for f in views}) == 1 and len({f[k].strides for f in views for k in (1, 2)}) == 1
        pitches = (views[0][0].strides[0] // views[0][0].itemsize, views[0][1].strides[0] // views[0][1].itemsize)
        for k, v in enumerate(extreme_fields(size)):
            f = FACTORS[k % 3]
            j = 1 + k % (f - 1)
            diff = same_planes(k_render(lib, *views, depth, f, j, v, 0, 0, 0, pitches), R.render(c, n, depth, f, j, v, 0, 0, 0))
            assert not diff, (size, k, diff)


@pytest.mark.parametrize("cls", [1, 4, 8])
@pytest.mark.parametrize("depth", [8, 10])
def test_vectors_with_misaligned_planes(lib, depth, cls):
    for size in SIZES[1:]:
        c, n = frames(size, depth, "noise")
        views = [view_of_class(f[0], cls) for f in (c, n)]
        assert views[0].strides == views[1].strides
        v0, v, D = k_vectors(lib, [views[0]], [views[1]], depth, views[0].strides[0] // views[0].itemsize)
        want = model_vectors(size, depth, "noise")
        assert np.array_equal(v0, want[0]) and np.array_equal(v, want[1]) and D == want[2], size


@functools.lru_cache(maxsize=None)
def hd_pair():
    """1920x1080, 8 bit: a pan by (10, -6) with a square that stands still in it"""
    c, n = pan_frames((1920, 1080), 8, (10, -6), seed=3, lo=90, hi=170)
    n = tuple(p.copy() for p in n)
    for a, b in zip(n, c):
        hh, ww = a.shape
        a[hh // 3:hh // 3 + hh // 5, ww // 3:ww // 3 + hh // 5] = b[hh // 3:hh // 3 + hh // 5, ww // 3:ww // 3 + hh // 5]
    return c, n, R.vectors(c[0], n[0], 8)


def test_vectors_equal_model_at_1080p(lib):
    """tile counts and index ranges of a real picture"""
    c, n, want = hd_pair()
    v0, v, D = k_vectors(lib, c, n, 8)
    assert np.array_equal(v0, want[0]) and np.array_equal(v, want[1]) and D == want[2]
    assert len(np.unique(want[1].reshape(-1, 2), axis=0)) > 1 and not R.is_cut(D, 10, 1920, 1080)


def test_render_equals_model_at_1080p(lib):
    c, n, (_, v, D) = hd_pair()
    diff = same_planes(k_render(lib, c, n, 8, 3, 2, v, D), R.render(c, n, 8, 3, 2, v, D))
    assert not diff, diff


# ------------------------------------------------------------------------------------------------ 2. sessions
def drain(enc):
    enc.flush()
    got = list(enc.packets())
    return b"".join(d for d, _, _ in got), [p for _, p, _ in got]


@functools.lru_cache(maxsize=None)
def reference_stream(depth, f, mode=0, n=N_FRAMES):
    """(stream, pts list) of a session fed the MODEL's pictures, display size, through mihevc_send_frame with the same pts"""
    from hevc_amd.encoder import Encoder
    with Encoder(cfg_of(depth), device=0) as enc:
        for pts, (y, u, v) in model_pictures(depth, f, mode, n):
            enc.send(np.ascontiguousarray(y), np.ascontiguousarray(u), np.ascontiguousarray(v), pts=pts)
        return drain(enc)


def test_the_clip_has_a_cut_and_moving_pairs():
    cl = clip(8)
    cuts = [R.is_cut(R.vectors(cl[k][0], cl[k + 1][0], 8)[2], 10, W, H) for k in range(N_FRAMES - 1)]
    assert cuts == [False] * (N_FRAMES - 3) + [True, False]
    assert R.vectors(cl[0][0], cl[1][0], 8)[1].any()


@pytest.mark.parametrize("route", ["sync", "async"])
@pytest.mark.parametrize("f", [2, 3])
@pytest.mark.parametrize("depth", [8, 10])
def test_session_stream_equals_the_model_fed_session(lib, depth, f, route):
    from hevc_amd.encoder import Encoder
    want, want_pts = reference_stream(depth, f)
    with Encoder(cfg_of(depth), device=0) as enc:
        assert enc.coded_size() == (104, 72)
        for i, src in enumerate(clip(depth)):
            enc.send_interpolate(*src, factor=f, asynchronous=route == "async")
            assert enc.stats().frames_in == f * i          # pictures, and a frame's come when the next frame arrives
        got, pts = drain(enc)
        assert enc.stats().frames_in == f * (N_FRAMES - 1) + 1
    assert len(want) > 200 and got == want
    assert pts == want_pts and sorted(pts) == list(range(f * (N_FRAMES - 1) + 1))


def test_blend_session_stream_equals_the_model_fed_session(lib):
    from hevc_amd.encoder import Encoder
    want, want_pts = reference_stream(8, 4, 1)
    with Encoder(cfg_of(8), device=0) as enc:
        for src in clip(8):
            enc.send_interpolate(*src, factor=4, mode="blend")
        got, pts = drain(enc)
    assert len(want) > 200 and got == want and pts == want_pts
    assert want != reference_stream(8, 4, 0)[0]


@pytest.fixture(scope="module")
def device_streams():
    """SHA-256 and pts of the streams of sessions fed from torch tensors, from ONE child process in which torch is initialised before the library
    (tests/mcfi_device_child.py says why): what this test is about is that order"""
    p = subprocess.run([sys.executable, "-s", "-m", "tests.mcfi_device_child"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    return json.loads(p.stdout[p.stdout.index("{"):])


@pytest.mark.parametrize("f", [2, 3])
@pytest.mark.parametrize("depth", [8, 10])
def test_session_fed_device_planes_equals_the_model_fed_session(lib, device_streams, depth, f):
    want, want_pts = reference_stream(depth, f)
    assert len(want) > 200 and device_streams[f"{depth}-{f}"] == [hashlib.sha256(want).hexdigest(), want_pts]


@pytest.mark.parametrize("depth", [8, 10])
def test_a_one_frame_clip(lib, depth):
    """flush produces the frame's own picture"""
    from hevc_amd.encoder import Encoder
    want, want_pts = reference_stream(depth, 2, 0, 1)
    with Encoder(cfg_of(depth), device=0) as enc:
        enc.send_interpolate(*clip(depth, 1)[0], factor=2)
        assert enc.stats().frames_in == 0
        got, pts = drain(enc)
        assert enc.stats().frames_in == 1
    assert len(want) > 100 and got == want and pts == want_pts == [0]


# ------------------------------------------------------------------------------------------------ 3. errors
def test_bad_calls_leave_the_session_usable(lib):
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    depth, f = 8, 2
    good = _lib.Interpolate(f, 0, 10)

    def send(enc, m, planes, pitch_y=W, pitch_c=W // 2, flags=0):
        return lib.mihevc_send_frame_interpolate(enc._s, None if m is None else C.byref(m), *planes, pitch_y, pitch_c, 99, flags)

    with Encoder(cfg_of(depth), device=0) as enc:
        for i, src in enumerate(clip(depth)):
            p = [q.ctypes.data for q in src]
            if i in (0, 2):          # before the first frame, and with a frame pending
                assert send(enc, None, p) == _lib.EINVAL
                for t in ((1, 0, 10), (5, 0, 10), (f, 2, 10), (f, -1, 10), (f, 0, -1), (f, 0, 256)):
                    assert send(enc, _lib.Interpolate(*t), p) == _lib.EINVAL, t
                for k in range(5):
                    bad = _lib.Interpolate(f, 0, 10)
                    bad.reserved[k] = 1
                    assert send(enc, bad, p) == _lib.EINVAL
                assert send(enc, good, p, pitch_y=W - 1) == _lib.EINVAL and send(enc, good, p, pitch_c=W // 2 - 1) == _lib.EINVAL
                assert send(enc, good, p, flags=4) == _lib.EINVAL
                for k in range(3):
                    assert send(enc, good, [None if j == k else q for j, q in enumerate(p)]) == _lib.EINVAL
            if i == 2:               # another factor or mode than the first frame's; and any other entry must wait for flush
                assert send(enc, _lib.Interpolate(3, 0, 10), p) == _lib.EINVAL and send(enc, _lib.Interpolate(f, 1, 10), p) == _lib.EINVAL
                assert lib.mihevc_send_frame(enc._s, *p, W, W // 2, 99) == _lib.ESTATE
                assert lib.mihevc_send_frame_async(enc._s, *p, W, W // 2, 99) == _lib.ESTATE
                assert lib.mihevc_send_frame_fmt(enc._s, C.byref(_lib.SrcFormat(422, 0, 8, 0)), *p, W, W // 2, 99, 0) == _lib.ESTATE
                assert lib.mihevc_send_frame_deint(enc._s, C.byref(_lib.Deint(1, 0)), *p, W, W // 2, 99, 0) == _lib.ESTATE
                assert lib.mihevc_send_frame_denoise(enc._s, C.byref(_lib.denoise_level(2)), *p, W, W // 2, 99, 0) == _lib.ESTATE
            enc.send_interpolate(*src, factor=f)
        stream, pts = drain(enc)
        assert send(enc, good, [q.ctypes.data for q in clip(depth)[0]]) == _lib.ESTATE          # after flush
    assert (stream, pts) == reference_stream(depth, f)


def test_interpolate_waits_while_a_denoised_frame_is_pending(lib):
    """mihevc_send_frame_interpolate returns MIHEVC_ESTATE while a denoised frame is pending, and the denoising session goes on as if it had not been called"""
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    outs = []
    for poke in (False, True):
        with Encoder(cfg_of(8), device=0) as enc:
            for i, src in enumerate(clip(8)):
                enc.send_denoise(*src, strength=2)
                if poke and i in (0, 3):
                    p = [q.ctypes.data for q in src]
                    assert lib.mihevc_send_frame_interpolate(enc._s, C.byref(_lib.Interpolate(2, 0, 10)), *p, W, W // 2, 99, 0) == _lib.ESTATE
            outs.append(drain(enc))
    assert len(outs[0][0]) > 200 and outs[0] == outs[1]


def test_sessions_the_entry_does_not_take(lib):
    """one band of a picture coded as two slices: MIHEVC_EINVAL, and the session codes on"""
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    y, u, v = (np.zeros(s, np.uint8) for s in ((64, W), (32, W // 2), (32, W // 2)))
    cfg = cfg_of(8)
    cfg.height = 64
    cfg.pic_height, cfg.slice_count, cfg.slice_index = 96, 2, 0
    cfg.slice_ctu_rows[0], cfg.slice_ctu_rows[1] = 2, 1
    cfg.rate_share_q16 = 43691
    with Encoder(cfg, device=0) as enc:
        assert lib.mihevc_send_frame_interpolate(enc._s, C.byref(_lib.Interpolate(2, 0, 10)), y.ctypes.data, u.ctypes.data, v.ctypes.data, W, W // 2, 0, 0) == _lib.EINVAL
        for k in range(3):
            enc.send(y, u, v)
        assert len(drain(enc)[0]) > 50
