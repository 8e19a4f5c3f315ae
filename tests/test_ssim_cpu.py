"""CPU: per-picture SSIM (mihevc_config.ssim).  The numpy reference of tests/ssim_ref.py against its own definition (hand forms, a literal per-window loop,
exact rationals, the textbook float form); the kernel programs of hevc_amd/csrc/kernels/ssim.h stepped on the CPU (tests/emu) against that reference, bit
for bit; configuration checks; the new entry points without a device; the SSIM column of tools/rd_curve.py --compare."""
import ctypes as C
import importlib.util
import json
import math
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from hevc_amd import _lib
from tests import ssim_ref as R
from tests import util

ROOT = Path(__file__).resolve().parents[1]
ONE = 1 << 32


def load_rd_curve():
    spec = importlib.util.spec_from_file_location("rd_curve", ROOT / "tools" / "rd_curve.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def shapes(w, h):
    return [(h, w), (h // 2, w // 2), (h // 2, w // 2)]


def dtype(bd):
    return np.uint8 if bd == 8 else np.uint16


def picture_pair(kind, w, h, bd, seed=0):
    """(source planes, reconstruction planes) of the coded size"""
    dt, top = dtype(bd), (1 << bd) - 1
    rng = np.random.default_rng(seed)
    a, b = [], []
    for s in shapes(w, h):
        if kind == "random":                     # two unrelated full-range pictures
            x, y = rng.integers(0, top + 1, s), rng.integers(0, top + 1, s)
        elif kind == "noise":                    # a reconstruction: the source plus a few levels of error
            x = rng.integers(0, top + 1, s)
            y = np.clip(x + rng.integers(-3, 4, s), 0, top)
        elif kind == "black_white":
            x, y = np.zeros(s, np.int64), np.full(s, top)
        elif kind == "checker":                  # against its inverse: every window anti-correlated
            yy, xx = np.mgrid[0:s[0], 0:s[1]]
            x = np.where((xx + yy) % 2 == 0, top, 0)
            y = top - x
        elif kind == "identical":
            x = rng.integers(0, top + 1, s)
            y = x
        else:
            raise ValueError(kind)
        a.append(np.ascontiguousarray(x.astype(dt)))
        b.append(np.ascontiguousarray(y.astype(dt)))
    return a, b


# ------------------------------------------------------------------------------------------------ 1. the reference against the definition
def test_constants():
    assert R.constants(8) == (26634, 239708)
    assert R.constants(10) == (428658, 3857925)
    for bd in (8, 10):
        peak = (1 << bd) - 1
        c1, c2 = R.constants(bd)
        assert abs(c1 - 4096 * (0.01 * peak) ** 2) <= 0.5 and abs(c2 - 4096 * (0.03 * peak) ** 2) <= 0.5


@pytest.mark.parametrize("w,h", [(8, 8), (64, 64), (136, 72), (104, 72)])
def test_window_count(w, h):
    a = np.zeros((h, w), np.uint8)
    assert R.window_q32(a, a, 8).shape == (h // 4 - 1, w // 4 - 1)
    assert R.plane(a, a, 8)[1] == R.window_count(w, h) == (w // 4 - 1) * (h // 4 - 1)


@pytest.mark.parametrize("bd", [8, 10])
def test_identical_planes_give_exactly_one(bd):
    a, _ = picture_pair("identical", 64, 48, bd, 3)
    q = R.window_q32(a[0], a[0], bd)
    assert np.all(q == ONE)
    assert R.plane(a[0], a[0], bd) == (ONE * q.size, q.size)
    assert R.value(*R.plane(a[0], a[0], bd)) == 1.0


@pytest.mark.parametrize("bd,want", [(8, 429450), (10, 429454)])
def test_black_against_white_is_the_hand_form(bd, want):
    peak = (1 << bd) - 1
    a, b = picture_pair("black_white", 32, 24, bd)
    q = R.window_q32(a[0], b[0], bd)
    c1, _ = R.constants(bd)
    hand = Fraction(c1, 4096 * peak * peak + c1) * ONE        # s1 = 0: f2 = g2 = c2 + ..., f1 = c1, g1 = (64 peak)^2 + c1; vars = 64 * 64 peak^2 - (64 peak)^2 = 0
    assert round(hand) == want
    assert np.all(q == want)


def test_checkerboard_against_its_inverse_is_negative():
    a, b = picture_pair("checker", 32, 32, 8)
    s, n = R.plane(a[0], b[0], 8)
    assert s < 0 and abs(R.value(s, n) - (-0.9964)) < 5e-5


def literal_windows(a, b, bd):
    """step by step, one window at a time, Python integers"""
    h, w = a.shape
    c1, c2 = R.constants(bd)
    out = []
    for wy in range(h // 4 - 1):
        for wx in range(w // 4 - 1):
            s1 = s2 = ss = s12 = 0
            for y in range(4 * wy, 4 * wy + 8):
                for x in range(4 * wx, 4 * wx + 8):
                    p, q = int(a[y, x]), int(b[y, x])
                    s1 += p; s2 += q; ss += p * p + q * q; s12 += p * q
            var = 64 * ss - s1 * s1 - s2 * s2
            covar = 64 * s12 - s1 * s2
            out.append((2 * s1 * s2 + c1, 2 * covar + c2, s1 * s1 + s2 * s2 + c1, var + c2))
    return out


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", ["random", "noise", "checker"])
def test_literal_loop_and_exact_rational(kind, bd):
    a, b = picture_pair(kind, 40, 24, bd, 7)
    got = R.window_q32(a[0], b[0], bd).reshape(-1)
    lit = literal_windows(a[0], b[0], bd)
    assert len(lit) == got.size
    for (f1, f2, g1, g2), q in zip(lit, got):
        assert max(abs(f1), abs(f2), g1, g2) < 1 << 53 and g1 > 0 and g2 > 0
        # the literal form: three float64 operations (Python floats are IEEE doubles), round half to even
        assert int(np.rint((float(f1) * float(f2)) / (float(g1) * float(g2)) * float(ONE))) == int(q)
        # against the exact rational: three roundings of 2^-53 relative each, scaled by 2^32, in front of the final rint
        exact = Fraction(f1 * f2, g1 * g2) * ONE
        assert abs(Fraction(int(q)) - exact) <= Fraction(1, 2) + Fraction(1, 1 << 19)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", ["random", "noise", "checker", "black_white"])
def test_textbook_float_form(kind, bd):
    """means, biased variances and covariance of every 8x8 window, C1 = (0.01 peak)^2 and C2 = (0.03 peak)^2 unrounded, float64.  c1, c2 are within 0.5 of
    4096 C1, 4096 C2; both ratios f1 / g1 and f2 / g2 lie in [-1, 1] with g1 >= c1 and g2 >= c2, so each moves by at most 1 / c; 1 % for the second-order
    term and float64 rounding"""
    peak = float((1 << bd) - 1)
    a, b = picture_pair(kind, 72, 40, bd, 5)
    x, y = a[0].astype(np.float64), b[0].astype(np.float64)
    q = R.window_q32(a[0], b[0], bd)
    c1, c2 = R.constants(bd)
    bound = 1.01 * (1.0 / c1 + 1.0 / c2)
    if bd == 8:
        assert abs(bound - 4.2e-5) < 1e-6
    C1, C2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    for wy in range(q.shape[0]):
        for wx in range(q.shape[1]):
            p, r = x[4 * wy:4 * wy + 8, 4 * wx:4 * wx + 8], y[4 * wy:4 * wy + 8, 4 * wx:4 * wx + 8]
            mx, my = p.mean(), r.mean()
            vx, vy, cov = (p * p).mean() - mx * mx, (r * r).mean() - my * my, (p * r).mean() - mx * my
            text = ((2 * mx * my + C1) * (2 * cov + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
            assert abs(q[wy, wx] / float(ONE) - text) <= bound, (wx, wy)


# ------------------------------------------------------------------------------------------------ 2. the kernel programs stepped on the CPU
@pytest.fixture(scope="module")
def emu():
    lib = util.stepped_library()
    lib.emu_ssim.argtypes = [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_void_p] * 2
    lib.emu_ssim_region.argtypes = [C.POINTER(C.c_int)] * 2
    return lib


def emu_ssim(emu, a, b, bd, order=0):
    h, w = a[0].shape
    s, n = np.full(3, -7, np.int64), np.zeros(3, np.int64)
    assert emu.emu_ssim(*[p.ctypes.data for p in a + b], w, h, bd, order, s.ctypes.data, n.ctypes.data) == 0
    return [int(v) for v in s], [int(v) for v in n]


def test_a_case_does_not_divide_into_the_workgroup_region(emu):
    rw, rh = C.c_int(), C.c_int()
    emu.emu_ssim_region(C.byref(rw), C.byref(rh))
    assert rw.value > 1 and rh.value > 1
    nx, ny = 136 // 4 - 1, 72 // 4 - 1          # luma windows of 136x72
    assert nx % rw.value and ny % rh.value and nx > rw.value and ny > rh.value      # partial regions at the right and at the bottom, behind whole ones
    assert (68 // 4 - 1) < rw.value              # and its chroma planes are narrower than one region


EMU_CASES = [(64, 64), (136, 72), (1920, 1080), (3840, 2160)]


@pytest.mark.parametrize("w,h", EMU_CASES, ids=[f"{w}x{h}" for w, h in EMU_CASES])
@pytest.mark.parametrize("bd", [8, 10])
def test_stepped_kernels_equal_reference(emu, w, h, bd):
    for k, kind in enumerate(("random", "noise", "black_white", "checker")):
        a, b = picture_pair(kind, w, h, bd, w + h + bd + k)
        want = R.picture(a, b, bd)
        assert want[1] == [R.window_count(*s[::-1]) for s in shapes(w, h)]
        assert emu_ssim(emu, a, b, bd) == want, kind
        if kind == "checker":
            assert all(v < 0 for v in want[0])


@pytest.mark.parametrize("bd", [8, 10])
def test_stepped_kernels_any_thread_order(emu, bd):
    for kind in ("random", "noise", "checker"):
        a, b = picture_pair(kind, 136, 72, bd, 11)
        want = R.picture(a, b, bd)
        for order in (0, 1, 2):
            assert emu_ssim(emu, a, b, bd, order) == want, (kind, order)


def test_stepped_kernels_full_range_ten_bit(emu):
    a, b = picture_pair("random", 264, 136, 10, 2)
    assert max(int(p.max()) for p in a + b) == 1023 and min(int(p.min()) for p in a + b) == 0
    assert emu_ssim(emu, a, b, 10) == R.picture(a, b, 10)
    a, b = picture_pair("identical", 264, 136, 10, 2)
    s, n = emu_ssim(emu, a, b, 10)
    assert s == [ONE * k for k in n]


# ------------------------------------------------------------------------------------------------ 3. configuration
def parameter_sets(cfg):
    buf = (C.c_uint8 * 4096)()
    n = _lib.load().mihevc_write_parameter_sets(C.byref(cfg), buf, 4096)
    return n, bytes(buf[:max(n, 0)])


def test_ssim_config_validation():
    assert _lib.default_config().ssim == 0
    for v, ok in [(0, True), (1, True), (2, False), (-1, False)]:
        cfg = _lib.default_config()
        cfg.ssim = v
        rc, _ = parameter_sets(cfg)
        assert (rc > 0) == ok and (ok or rc == _lib.EINVAL), (v, rc)
    cfg = _lib.default_config()
    cfg.height, cfg.pic_height, cfg.slice_count, cfg.slice_index = 544, 1080, 2, 0
    cfg.slice_ctu_rows[0], cfg.slice_ctu_rows[1] = 17, 17
    assert parameter_sets(cfg)[0] > 0
    cfg.ssim = 1
    assert parameter_sets(cfg)[0] == _lib.EINVAL


def test_ssim_does_not_touch_the_parameter_sets():
    outs = []
    for v in (0, 1):
        cfg = _lib.default_config()
        cfg.ssim = v
        outs.append(parameter_sets(cfg)[1])
    assert outs[0] and outs[0] == outs[1]


def test_config_for_passes_ssim_through():
    import inspect
    from hevc_amd import encoder
    from hevc_amd.probe import VideoInfo
    assert inspect.signature(encoder.config_for).parameters["ssim"].default == 0
    info = VideoInfo(1920, 1080, 30.0, "bt709", "bt709", "bt709", "yuv420p", "", "", 2)
    assert encoder.config_for(info, 19, 2940, 3528, 90, "4.0", "main").ssim == 0
    assert encoder.config_for(info, 19, 2940, 3528, 90, "4.0", "main", ssim=1).ssim == 1


def test_stats_mirror_ends_with_the_ssim_sums():
    assert [f[0] for f in _lib.Stats._fields_[-3:]] == ["ssim_y", "ssim_u", "ssim_v"]
    assert _lib.Config._fields_[-1][0] == "ssim"
    assert _lib.load().mihevc_abi_version() == 6


# ------------------------------------------------------------------------------------------------ 4. the entry points without a device
def test_entry_points_reject_bad_arguments():
    lib = _lib.load()
    sse = (C.c_uint64 * 3)()
    assert lib.mihevc_get_frame_quality(None, 0, sse, None, None) == _lib.EINVAL
    a, b = picture_pair("noise", 64, 64, 8)
    s, n = (C.c_int64 * 3)(), (C.c_int64 * 3)()
    args = [p.ctypes.data for p in a + b]
    assert lib.mihevc_k_ssim(0, *args, 60, 64, 8, s, n) == _lib.EINVAL
    assert lib.mihevc_k_ssim(0, *args, 64, 64, 9, s, n) == _lib.EINVAL
    assert lib.mihevc_k_ssim(0, None, *args[1:], 64, 64, 8, s, n) == _lib.EINVAL


@pytest.mark.skipif(_lib.load().mihevc_device_count() > 0, reason="a GPU is present")
def test_no_gpu_means_loud_failure():
    lib = _lib.load()
    a, b = picture_pair("noise", 64, 64, 8)
    s, n = (C.c_int64 * 3)(), (C.c_int64 * 3)()
    assert lib.mihevc_k_ssim(0, *[p.ctypes.data for p in a + b], 64, 64, 8, s, n) == _lib.ENODEV
    cfg = _lib.default_config()
    cfg.ssim = 1
    h = C.c_void_p()
    assert lib.mihevc_open(C.byref(cfg), 0, C.byref(h)) == _lib.ENODEV and not h.value


# ------------------------------------------------------------------------------------------------ 5. tools/rd_curve.py --compare
def synthetic_run(shift=0.0, ssim=True, clips=("motion", "stress")):
    """points on log(kbps) = 5 + 0.08 q + 0.002 q^2 (+ shift) for q = PSNR and for q = SSIM in dB: at every quality the second run's rate is
    exp(shift) times the first's, so the Bjontegaard integral (an average of the log-rate difference over quality) is exp(shift) - 1 by either column"""
    run = {"clips": {}}
    for k, clip in enumerate(clips):
        pts = []
        for i, q in enumerate((30.0 + k, 33.5 + k, 37.0 + k, 41.0 + k)):
            p = {"qp": 37 - 5 * i, "kbps": math.exp(5 + 0.08 * q + 0.002 * q * q + shift), "psnr_y": q}
            if ssim:
                d = q - 22.0                  # SSIM in dB along the same curve, moved: log(kbps) = 5 + 0.08 (d + 22) + ...: still a quadratic in d
                p["ssim_y_db"] = d
                p["ssim_y"] = 1 - 10 ** (-d / 10)
            pts.append(p)
        run["clips"][clip] = {"points": pts}
    return run


def test_compare_bd_rate_by_ssim_is_the_known_shift():
    rd = load_rd_curve()
    shift = math.log(1.07)
    out = rd.compare(synthetic_run(), synthetic_run(shift))
    for clip in ("motion", "stress"):
        assert abs(out[clip]["bd_rate_ssim_pct"] - 7.0) <= 0.011 and abs(out[clip]["bd_rate_pct"] - 7.0) <= 0.011      # (results are rounded to 0.01)
    assert abs(out["mean_bd_rate_ssim_pct"] - 7.0) <= 0.011
    same = rd.compare(synthetic_run(), synthetic_run())
    assert same["motion"]["bd_rate_ssim_pct"] == 0 and same["mean_bd_rate_ssim_pct"] == 0


def test_compare_without_an_ssim_column_gives_none():
    rd = load_rd_curve()
    for a, b in ((synthetic_run(ssim=False), synthetic_run(0.1)), (synthetic_run(), synthetic_run(0.1, ssim=False))):
        out = rd.compare(a, b)
        assert out["motion"]["bd_rate_ssim_pct"] is None and out["mean_bd_rate_ssim_pct"] is None
        assert out["motion"]["bd_rate_pct"] is not None and out["mean_bd_rate_pct"] is not None


def test_compare_of_stored_runs_is_what_it_was(tmp_path):
    rd = load_rd_curve()
    a, b = (json.load(open(ROOT / "profiles" / "r03" / n)) for n in ("rd_base.json", "rd_bframes1.json"))
    out = rd.compare(a, b)
    want, rates = {}, []
    for clip in a["clips"]:
        if clip not in b["clips"]:
            continue
        pa, pb = ([(p["kbps"], p["psnr_y"]) for p in x["clips"][clip]["points"]] for x in (a, b))
        want[clip] = {"bd_rate_pct": round(rd.bd_rate(pa, pb), 2), "bd_psnr_db": round(rd.bd_psnr(pa, pb), 3)}
        rates.append(want[clip]["bd_rate_pct"])
    assert want
    for clip, w in want.items():
        assert {k: out[clip][k] for k in w} == w
        assert out[clip]["bd_rate_ssim_pct"] is None
    assert out["mean_bd_rate_pct"] == round(float(np.mean(rates)), 2) and out["mean_bd_rate_ssim_pct"] is None
    assert set(out) == set(want) | {"mean_bd_rate_pct", "mean_bd_rate_ssim_pct"}
    # and through the command line
    import subprocess
    import sys
    cli = subprocess.run([sys.executable, str(ROOT / "tools" / "rd_curve.py"), "--compare", str(ROOT / "profiles" / "r03" / "rd_base.json"),
                          str(ROOT / "profiles" / "r03" / "rd_bframes1.json")], capture_output=True, text=True, check=True)
    assert json.loads(cli.stdout) == out
