"""What the tests of the two source converters (test_ingest_cpu, test_ingest_rgb_cpu, test_gpu_ingest, test_gpu_ingest_rgb) share: plane comparison, the
stand-in ffmpeg of the pipe front end, the small session of the GPU tests and source planes of a chosen alignment class."""
import numpy as np
import pytest

from hevc_amd import probe
from tests.test_host_robustness import FAKE_FFMPEG


def same_planes(got, want):
    for name, g, w in zip("Y Cb Cr".split(), got, want):
        if not np.array_equal(g, w):
            ys, xs = np.nonzero(g != w)
            return f"{name}: {len(ys)} samples differ, first at x={xs[0]} y={ys[0]}: {g[ys[0], xs[0]]} vs {w[ys[0], xs[0]]}"
    return ""


# ------------------------------------------------------------------------------------------------ the ffmpeg pipe front end
@pytest.fixture
def fake_ffmpeg(tmp_path, monkeypatch):
    b = tmp_path / "bin"
    b.mkdir()
    f = b / "ffmpeg"
    f.write_text(FAKE_FFMPEG)
    f.chmod(0o755)
    monkeypatch.setenv("PATH", f"{b}:/usr/bin:/bin")
    monkeypatch.setenv("FAKE_LOG", str(tmp_path / "ffmpeg.log"))
    return tmp_path / "ffmpeg.log"


def info(pix, w=64, h=48, n=3, matrix="bt709"):
    return probe.VideoInfo(w, h, 30.0, "bt709", "bt709", matrix, pix, "", "", 0, False, "eng", n, n / 30.0)


def pix_fmt_asked(log):
    argv = log.read_text().split("\n")[-2].split()
    return argv[argv.index("-pix_fmt") + 1]


# ------------------------------------------------------------------------------------------------ GPU sessions
W, H, N = 100, 70, 5


def base_cfg(depth):
    from hevc_amd import _lib
    cfg = _lib.default_config()
    cfg.width, cfg.height, cfg.bit_depth, cfg.keyint, cfg.min_keyint, cfg.scenecut, cfg.qp, cfg.me_range, cfg.gops_in_flight = W, H, depth, 3, 2, 0, 28, 12, 1
    cfg.level_idc = 93
    return cfg


def drain(enc, keep_recon=False):
    enc.flush()
    stream = b"".join(d for d, _, _ in enc.packets())
    return (stream, [enc.recon(i) for i in range(N)]) if keep_recon else stream


def device_planes(planes):
    import torch
    out = [None if p is None else torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p).cuda() for p in planes]
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ alignment classes
def alignment_class(n):
    """of an address or a pitch in bytes: the widest chunk it allows (ingest_align): the largest of 16, 8, 4 that divides it, else 1"""
    return next((c for c in (16, 8, 4) if n % c == 0), 1)


def view_of_class(p, cls):
    """A copy of plane `p` whose address modulo 16 and whose pitch in bytes have exactly the alignment `cls` (1, 4 or 8) and no more; class 1: one element past
    a 16-byte boundary, odd pitch.  The start element comes from the buffer's real address.  Planes of one shape get one pitch.  The view keeps its buffer alive"""
    es = p.itemsize
    unit = max(cls // es, 1)                                      # elements
    pitch = (p.shape[1] // unit + 1) * unit
    pitch += unit if (pitch // unit) % 2 == 0 else 0              # an odd multiple: not a multiple of the next power of two
    buf = np.zeros(pitch * p.shape[0] + 16 + unit, p.dtype)
    start = (-buf.ctypes.data % 16) // es + unit                  # `unit` elements past a 16-byte boundary
    v = np.lib.stride_tricks.as_strided(buf[start:], p.shape, (pitch * es, es))
    v[...] = p
    return v
