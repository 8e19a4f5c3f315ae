"""GPU (-m gpu): mihevc_receive_packets hands out what mihevc_receive_packet hands out, a batch at a time (include/mihevc.h).

Two sessions code the same ten pictures (128x64, keyint 4, two GOP lanes); one is drained packet by packet, the other through the batch call with max 1,
3 and 64 and with the two calls mixed: bytes, pts, dts and key flags must be equal.  Return codes follow the one-packet call: MIHEVC_EAGAIN before
flush with nothing ready, MIHEVC_EOF once flushed and drained (and again on the next call), MIHEVC_EINVAL for max <= 0 or a NULL data / size array with
the session still usable.  The pointers of one batch are read after the call that returned them and before the next receive call: that is how long they
live.  One case runs with bframes = 1, where dts != pts."""
import ctypes as C
import functools

import pytest

from tests import util

pytestmark = pytest.mark.gpu

W, H, N = 128, 64, 10


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


@functools.lru_cache(maxsize=None)
def clip():
    return tuple(tuple(util.planes(util.synth_frame(H, W, seed=3, shift=(2 * i, i)), 8)) for i in range(N))


def make_cfg(bframes=0):
    from hevc_amd import _lib
    cfg = _lib.default_config()
    cfg.width, cfg.height, cfg.keyint, cfg.min_keyint, cfg.gops_in_flight, cfg.scenecut, cfg.qp, cfg.me_range, cfg.level_idc = W, H, 4, 2, 2, 0, 28, 8, 93
    cfg.bframes = bframes
    return cfg


class Session:
    """a raw session (no hevc_amd.encoder on the way: the C calls themselves are under test)"""

    def __init__(self, lib, cfg):
        self.lib, self.s = lib, C.c_void_p()
        assert lib.mihevc_open(C.byref(cfg), 0, C.byref(self.s)) == 0

    def close(self):
        self.lib.mihevc_close(self.s)

    def send(self, i):
        y, u, v = clip()[i]
        assert self.lib.mihevc_send_frame(self.s, y.ctypes.data, u.ctypes.data, v.ctypes.data, W, W // 2, i) == 0

    def flush(self):
        assert self.lib.mihevc_flush(self.s) == 0

    def one(self):
        """mihevc_receive_packet -> (bytes, pts, dts, key) or the negative code"""
        data, size, pts, dts, key = C.POINTER(C.c_uint8)(), C.c_size_t(), C.c_int64(), C.c_int64(), C.c_int()
        rc = self.lib.mihevc_receive_packet(self.s, C.byref(data), C.byref(size), C.byref(pts), C.byref(dts), C.byref(key))
        return rc if rc else (C.string_at(data, size.value), pts.value, dts.value, key.value)

    def batch(self, max_):
        """mihevc_receive_packets -> list of (bytes, pts, dts, key) or the negative code.  Arrays of 64 with a guard value behind what may be written"""
        data, size, pts, dts, key = (C.c_void_p * 65)(), (C.c_size_t * 65)(), (C.c_int64 * 65)(), (C.c_int64 * 65)(), (C.c_int * 65)()
        guard = min(max(max_, 0), 64)
        size[guard], pts[guard], key[guard] = 0xabcdef, -77, 1234
        n = self.lib.mihevc_receive_packets(self.s, max_, data, size, pts, dts, key)
        assert (size[guard], pts[guard], key[guard]) == (0xabcdef, -77, 1234), "the call wrote past max"
        if n <= 0:
            return n
        assert n <= max_
        # every pointer of the batch is read here, after the call has returned and before the next receive call
        return [(C.string_at(data[i], size[i]), pts[i], dts[i], key[i]) for i in range(n)]


def coded(lib, cfg, drain):
    """the clip through one session; drain(session) -> the packets, called once before flush (with everything sent) and once behind it"""
    s = Session(lib, cfg)
    try:
        for i in range(N):
            s.send(i)
        got = drain(s, False)
        s.flush()
        got += drain(s, True)
        return got
    finally:
        s.close()


def drain_single(s, flushed):
    from hevc_amd import _lib
    out = []
    while True:
        r = s.one()
        if isinstance(r, int):
            assert r == (_lib.EOF if flushed else _lib.EAGAIN)
            return out
        out.append(r)


def drain_batch(max_):
    def drain(s, flushed):
        from hevc_amd import _lib
        out = []
        while True:
            r = s.batch(max_)
            if isinstance(r, int):
                assert r == (_lib.EOF if flushed else _lib.EAGAIN)
                if flushed:
                    assert s.batch(max_) == _lib.EOF and s.one() == _lib.EOF, "EOF must repeat, from either call"
                return out
            out += r
    return drain


def drain_mixed(s, flushed):
    """batch of 2, one packet, batch of 3, one packet, ..."""
    from hevc_amd import _lib
    out, k = [], 0
    while True:
        r = s.one() if k % 2 else s.batch(2 + (k // 2) % 2)
        k += 1
        if isinstance(r, int):
            assert r == (_lib.EOF if flushed else _lib.EAGAIN)
            return out
        out += [r] if isinstance(r, tuple) else r


@pytest.fixture(scope="module")
def reference(lib):
    return {bf: coded(lib, make_cfg(bf), drain_single) for bf in (0, 1)}


def check(got, want):
    assert len(want) == N and len(got) == N
    for i, (a, b) in enumerate(zip(got, want)):
        assert a[1:] == b[1:], f"packet {i}: pts / dts / key {a[1:]} != {b[1:]}"
        assert a[0] == b[0], f"packet {i}: {len(a[0])} bytes from the batch call, {len(b[0])} from the one-packet call, or other bytes"


def test_reference_is_what_the_cases_need(reference):
    for bf, pk in reference.items():
        assert [p[3] for p in pk].count(1) >= 2 and pk[0][3] == 1 and not all(p[3] for p in pk), "closed GOPs of up to 4 pictures: key and other packets"
        assert all(len(p[0]) > 8 and p[0][:4] == b"\x00\x00\x00\x01" for p in pk)
        assert all(p[2] <= p[1] for p in pk)
    assert all(p[1] == p[2] for p in reference[0]) and sorted(p[1] for p in reference[0]) == [p[1] for p in reference[0]]
    assert any(p[1] != p[2] for p in reference[1]), "bframes = 1 must reorder: dts != pts somewhere"


@pytest.mark.parametrize("max_", [1, 3, 64])
def test_batches_equal_single_packets(lib, reference, max_):
    check(coded(lib, make_cfg(), drain_batch(max_)), reference[0])


def test_mixed_with_single_receives(lib, reference):
    check(coded(lib, make_cfg(), drain_mixed), reference[0])


def test_b_pictures_dts(lib, reference):
    check(coded(lib, make_cfg(1), drain_batch(3)), reference[1])
    check(coded(lib, make_cfg(1), drain_mixed), reference[1])


def test_bad_arguments_leave_the_session_usable(lib, reference):
    from hevc_amd import _lib

    def drain(s, flushed):
        data, size = (C.c_void_p * 4)(), (C.c_size_t * 4)()
        assert s.batch(0) == _lib.EINVAL and s.batch(-1) == _lib.EINVAL
        assert lib.mihevc_receive_packets(s.s, 4, None, size, None, None, None) == _lib.EINVAL
        assert lib.mihevc_receive_packets(s.s, 4, data, None, None, None, None) == _lib.EINVAL
        assert lib.mihevc_receive_packets(None, 4, data, size, None, None, None) == _lib.EINVAL
        return drain_batch(64)(s, flushed)
    check(coded(lib, make_cfg(), drain), reference[0])


def test_optional_arrays_may_be_null(lib, reference):
    """pts, dts and keyframe are optional, as in the one-packet call"""
    def drain(s, flushed):
        data, size = (C.c_void_p * 64)(), (C.c_size_t * 64)()
        n = lib.mihevc_receive_packets(s.s, 64, data, size, None, None, None)
        return [C.string_at(data[i], size[i]) for i in range(max(n, 0))]
    s = coded(lib, make_cfg(), drain)
    assert s == [p[0] for p in reference[0]]


def test_encoder_generators_use_the_batch_and_keep_leftovers(lib, reference):
    """hevc_amd.encoder: packets() / packets_dts() yield the tuples they always did, and a caller that stops early finds the rest in its next call"""
    from hevc_amd.encoder import Encoder
    with Encoder(make_cfg(1), device=0) as enc:
        for i in range(N):
            enc.send(*clip()[i])
        enc.flush()
        it = enc.packets_dts()
        first = [next(it) for _ in range(3)]
        it.close()
        rest = list(enc.packets())
        assert list(enc.packets()) == [] and list(enc.packets_dts()) == []
    want = reference[1]
    assert first == [(d, p, bool(k), t) for d, p, t, k in want[:3]]
    assert rest == [(d, p, bool(k)) for d, p, t, k in want[3:]]
    assert all(type(k) is bool and type(p) is int for _, p, k in rest)
