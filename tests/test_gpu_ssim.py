"""GPU (-m gpu): per-picture SSIM and squared error (mihevc_config.ssim, mihevc_get_frame_quality) on an MI355X.  The kernels alone (mihevc_k_ssim) against
the numpy reference of tests/ssim_ref.py, bit for bit; sessions: every output picture's squared error and SSIM sums equal numpy's of (edge-extended
source, the session's own reconstruction), in display order, and the session totals are their sums; ssim = 1 changes no byte of the stream and no sample of
a reconstruction; configuration and state errors; tools/rd_curve.py end to end."""
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import ssim_ref as R
from tests import util
from tests.test_ssim_cpu import picture_pair

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
ONE = float(1 << 32)


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


# ------------------------------------------------------------------------------------------------ 6. the kernels alone
def k_ssim(lib, a, b, bd):
    h, w = a[0].shape
    s, n = (C.c_int64 * 3)(-7, -7, -7), (C.c_int64 * 3)()
    assert lib.mihevc_k_ssim(0, *[p.ctypes.data for p in a + b], w, h, bd, s, n) == 0
    return [int(v) for v in s], [int(v) for v in n]


STAGE = [(64, 64), (136, 72), (1920, 1080), (3840, 2160)]


@pytest.mark.parametrize("w,h", STAGE, ids=[f"{w}x{h}" for w, h in STAGE])
@pytest.mark.parametrize("bd", [8, 10])
def test_stage_equals_reference(lib, w, h, bd):
    for k, kind in enumerate(("random", "noise", "black_white", "checker")):
        a, b = picture_pair(kind, w, h, bd, w + h + bd + k)
        want, got = R.picture(a, b, bd), k_ssim(lib, a, b, bd)
        print(f"{w}x{h} {bd} bit {kind}: device {got[0]} reference {want[0]} windows {want[1]}")
        assert got == want, kind
        if kind == "checker":
            assert all(v < 0 for v in got[0])


def test_stage_identical_and_full_range_ten_bit(lib):
    a, b = picture_pair("random", 264, 136, 10, 2)
    assert max(int(p.max()) for p in a + b) == 1023 and min(int(p.min()) for p in a + b) == 0
    assert k_ssim(lib, a, b, 10) == R.picture(a, b, 10)
    a, b = picture_pair("identical", 264, 136, 10, 2)
    s, n = k_ssim(lib, a, b, 10)
    assert s == [(1 << 32) * k for k in n]


# ------------------------------------------------------------------------------------------------ 7. sessions
def base_cfg(w, h, bd=8, **kw):
    from hevc_amd import _lib
    cfg = _lib.default_config()
    cfg.width, cfg.height, cfg.bit_depth, cfg.keyint, cfg.min_keyint, cfg.scenecut, cfg.qp, cfg.me_range, cfg.gops_in_flight = w, h, bd, 30, 2, 0, 30, 12, 1
    cfg.level_idc = 93
    if bd == 10:      # Main10 HDR10 (core/utils.py:58-69)
        cfg.colour_primaries, cfg.transfer, cfg.matrix, cfg.hdr10, cfg.aud, cfg.repeat_headers, cfg.hrd, cfg.chroma_loc = 9, 16, 9, 1, 1, 1, 1, 0
    cfg.ssim = 1
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def clip(w, h, bd, n, cut=None):
    """n pictures of a translating scene; cut: another scene from that picture on, moving at half the speed: the cut detector wants a picture difference of
    1.8 times the ordinary one (numpy, every 4th sample of 416x240: 28 grey levels at the cut against 10 - 12 between neighbours)"""
    if cut is None:
        return [util.synth_frame(h, w, seed=4, shift=(2 * i, i), bit_depth=bd) for i in range(n)]
    return [util.synth_frame(h, w, seed=40 + (i >= cut), shift=(i, i // 2), bit_depth=bd) for i in range(n)]


def run_session(cfg, frames, device_planes=False):
    """-> (packets, headers, reconstructions, frame_quality per picture, stats, slice types)"""
    from hevc_amd.encoder import Encoder
    bd, n = cfg.bit_depth, len(frames)
    hip, dev = None, []
    if device_planes:      # the frames in device memory through the HIP runtime the library links: the session codes straight from these planes
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        assert hip.hipSetDevice(0) == 0
    try:
        with Encoder(cfg, device=0, keep_recon=True) as enc:
            for i, f in enumerate(frames):
                pl = util.planes(f, bd)
                if device_planes:
                    row = []
                    for p in pl:
                        d = C.c_void_p()
                        assert hip.hipMalloc(C.byref(d), p.nbytes) == 0
                        assert hip.hipMemcpy(d, p.ctypes.data_as(C.c_void_p), p.nbytes, 1) == 0      # hipMemcpyHostToDevice
                        row.append(d.value)
                    dev.append(row)
                    enc.send_device(row[0], row[1], row[2], cfg.width, cfg.width // 2, pts=i)
                else:
                    enc.send(*pl)
            enc.flush()
            pk = list(enc.packets())
            recs = [enc.recon(i) for i in range(n)]
            fq = [enc.frame_quality(i) for i in range(n)]
            st = enc.stats()
            types = [enc.frame_info(i)[1] for i in range(n)]
            return pk, enc.headers(), recs, fq, st, types, enc.coded_size()
    finally:
        for row in dev:
            for d in row:
                hip.hipFree(d)


def check_quality(cfg, frames, recs, fq, st, coded):
    bd, n = cfg.bit_depth, len(frames)
    cw, ch = coded
    tot_sse, tot_q, win = [0, 0, 0], [0, 0, 0], None
    for i, f in enumerate(frames):
        src = [R.extend(p, cw >> (c > 0), ch >> (c > 0)) for c, p in enumerate(util.planes(f, bd))]
        rec = [np.asarray(p) for p in recs[i]]
        sse = [int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) for a, b in zip(src, rec)]
        q32, win = R.picture(src, rec, bd)
        print(f"picture {i}: sse {fq[i]['sse']} / numpy {sse}; ssim_q32 {fq[i]['ssim_q32']} / reference {q32}")
        assert fq[i]["sse"] == sse, f"picture {i}: squared error"
        assert fq[i]["ssim_q32"] == q32 and fq[i]["ssim_windows"] == win, f"picture {i}: SSIM sums"
        assert fq[i]["ssim"] == [q / (k * ONE) for q, k in zip(q32, win)]
        peak = (1 << bd) - 1
        for c in range(3):
            assert abs(fq[i]["psnr"][c] - util.psnr(src[c], rec[c], peak)) < 1e-9
        tot_sse = [a + b for a, b in zip(tot_sse, sse)]
        tot_q = [a + b for a, b in zip(tot_q, q32)]
    assert st.frames_out == n
    assert [st.sse_y, st.sse_u, st.sse_v] == [float(v) for v in tot_sse]
    assert [st.ssim_y, st.ssim_u, st.ssim_v] == [q / (k * ONE) for q, k in zip(tot_q, win)]
    per_picture = [sum(fq[i]["ssim"][c] for i in range(n)) for c in range(3)]                   # the same sum formed from the per-picture doubles
    assert all(abs(a - b) < 1e-9 * n for a, b in zip([st.ssim_y, st.ssim_u, st.ssim_v], per_picture))
    assert all(0 < v / n <= 1 for v in per_picture)


SESSIONS = {
    "ippp-100x70": dict(w=100, h=70, n=6),                                                      # coded 104x72: the margin is the session's edge replication
    "lanes-scenecut-416x240": dict(w=416, h=240, n=20, cut=5, kw=dict(keyint=8, gops_in_flight=3, scenecut=1)),
    "hdr10": dict(w=320, h=192, bd=10, n=5),
    "bframes": dict(w=320, h=192, n=9, kw=dict(bframes=1, keyint=9)),
    "no-sao": dict(w=320, h=192, n=5, kw=dict(sao=0)),
    "p-tiles": dict(w=512, h=64, n=4, kw=dict(p_tiles=1, level_idc=120)),
    "device-planes": dict(w=320, h=192, n=6, device_planes=True, kw=dict(keyint=3, gops_in_flight=2)),
}


@pytest.mark.parametrize("name", list(SESSIONS))
def test_session_quality_per_picture(lib, name):
    from hevc_amd import _lib
    c = SESSIONS[name]
    bd = c.get("bd", 8)
    cfg = base_cfg(c["w"], c["h"], bd, **c.get("kw", {}))
    frames = clip(c["w"], c["h"], bd, c["n"], c.get("cut"))
    pk, _, recs, fq, st, types, coded = run_session(cfg, frames, c.get("device_planes", False))
    assert len(pk) == c["n"]
    if name == "ippp-100x70":
        assert coded == (104, 72) and types == [2] + [1] * 5
    if name == "lanes-scenecut-416x240":
        assert types[c["cut"]] == 2 and types.count(2) >= 3, types
    if name == "bframes":
        assert 0 in types, types
    if name == "p-tiles":
        assert _lib.p_tile_grid(cfg) == (2, 1)
    check_quality(cfg, frames, recs, fq, st, coded)


# ------------------------------------------------------------------------------------------------ 8. neutrality
@pytest.mark.parametrize("pic_hash,bframes", [(0, 0), (2, 1)], ids=["plain", "with-crc-and-b"])
def test_ssim_changes_no_byte(lib, pic_hash, bframes):
    w, h, n = 416, 240, 10
    frames = clip(w, h, 8, n)
    out = []
    for ssim in (0, 1):
        cfg = base_cfg(w, h, 8, ssim=ssim, pic_hash=pic_hash, bframes=bframes, keyint=5, gops_in_flight=2)
        pk, hdr, recs, fq, st, types, coded = run_session(cfg, frames)
        out.append((pk, hdr, [[p.tobytes() for p in r] for r in recs], types, [q["sse"] for q in fq], (st.sse_y, st.sse_u, st.sse_v, st.bytes_out)))
        if ssim:
            check_quality(cfg, frames, recs, fq, st, coded)
        else:
            assert (st.ssim_y, st.ssim_u, st.ssim_v) == (0.0, 0.0, 0.0) and all(q["ssim"] is None for q in fq)
    assert out[0] == out[1]


# ------------------------------------------------------------------------------------------------ 9. configuration and state
def test_sliced_sessions_refuse_ssim_and_plain_sessions_refuse_the_ssim_outputs(lib):
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    cfg = _lib.default_config()
    cfg.height, cfg.pic_height, cfg.slice_count, cfg.slice_index, cfg.ssim = 544, 1080, 2, 0, 1
    cfg.slice_ctu_rows[0], cfg.slice_ctu_rows[1] = 17, 17
    s = C.c_void_p()
    assert lib.mihevc_open(C.byref(cfg), 0, C.byref(s)) == _lib.EINVAL and not s.value
    for v in (2, -1):
        cfg = base_cfg(320, 192, ssim=v)
        assert lib.mihevc_open(C.byref(cfg), 0, C.byref(s)) == _lib.EINVAL and not s.value
    w, h, n = 320, 192, 3
    cfg = base_cfg(w, h, ssim=0)
    frames = clip(w, h, 8, n)
    with Encoder(cfg, device=0, keep_recon=True) as enc:
        sse, q32, win = (C.c_uint64 * 3)(), (C.c_int64 * 3)(), (C.c_int64 * 3)()
        assert lib.mihevc_get_frame_quality(enc._s, 0, sse, None, None) == _lib.ESTATE          # no such picture yet
        for f in frames:
            enc.send(*util.planes(f, 8))
        enc.flush()
        assert len(list(enc.packets())) == n
        for i in range(n):
            assert lib.mihevc_get_frame_quality(enc._s, i, sse, None, None) == 0
            rec = enc.recon(i)
            want = [int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) for a, b in zip(util.planes(frames[i], 8), rec)]
            assert [int(v) for v in sse] == want
            assert lib.mihevc_get_frame_quality(enc._s, i, sse, q32, None) == _lib.ESTATE
            assert lib.mihevc_get_frame_quality(enc._s, i, None, None, win) == _lib.ESTATE
            assert enc.frame_quality(i)["ssim"] is None and enc.frame_quality(i)["sse"] == want
        assert lib.mihevc_get_frame_quality(enc._s, n, sse, None, None) == _lib.ESTATE
        assert lib.mihevc_get_frame_quality(enc._s, -1, sse, None, None) == _lib.ESTATE


# ------------------------------------------------------------------------------------------------ 10. tools/rd_curve.py end to end
def test_rd_curve_carries_ssim(lib, tmp_path):
    out = tmp_path / "rd.json"
    p = subprocess.run([sys.executable, str(ROOT / "tools" / "rd_curve.py"), "--out", str(out), "--width", "416", "--height", "240", "--frames", "12", "--keyint", "12",
                        "--clips", "motion"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(out.read_text())
    pts = sorted(res["clips"]["motion"]["points"], key=lambda q: q["qp"])
    assert [q["qp"] for q in pts] == [22, 27, 32, 37]
    print([(q["qp"], q["kbps"], q["psnr_y"], q["ssim_y"], q["ssim_y_db"]) for q in pts])
    assert all(0 < q["ssim_y"] <= 1 for q in pts)
    assert all(a["ssim_y"] > b["ssim_y"] and a["ssim_y_db"] > b["ssim_y_db"] for a, b in zip(pts, pts[1:]))      # rising with falling QP
    assert all(abs(q["ssim_y_db"] - (-10 * np.log10(1 - q["ssim_y"]))) < 0.01 for q in pts)
    from tests.test_ssim_cpu import load_rd_curve
    same = load_rd_curve().compare(res, res)
    assert same["motion"]["bd_rate_ssim_pct"] == 0 and same["mean_bd_rate_ssim_pct"] == 0
