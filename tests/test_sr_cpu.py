"""CPU: the learned super-resolution path without a device.  1. the model tests/sr_ref.py pinned against torch's own operators and a hand-worked network;
2. the host side of csrc/sr_net.h (half rounding, packing, counts, memory); 3. the stepped k_sr_conv bit for bit against an integer numpy convolution (== on
values that are exact in fp32 and half whatever the order of summation); 4. the stepped k_sr_input bit for bit against numpy; 5. the whole network stepped,
against the float64 model within twice the half model's own error; 6. the stand-alone AddressSanitizer / UBSan program; 7. the entries without a device.

The activation of the exact tests runs with the exact slope 0.25 passed through the stage entry; the real slope 0.2 is what the network tests run."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from hevc_amd import _lib
from tests import sr_common as S
from tests import sr_ref as R
from tests import util

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def emu():
    return util.stepped_library()


# ------------------------------------------------------------------------------------------------ 1. the model itself
def test_unshuffle_and_enlargement_are_torchs():
    import torch
    import torch.nn.functional as F
    x = torch.arange(3 * 6 * 8, dtype=torch.float32).reshape(3, 6, 8)
    assert torch.equal(R.pixel_unshuffle(x), F.pixel_unshuffle(x[None], 2)[0])
    assert torch.equal(R.nearest2x(x), F.interpolate(x[None], scale_factor=2, mode="nearest")[0])


def test_model_by_hand_on_a_network_of_chosen_taps():
    """one block, every weight zero except: conv_first copies R into feature 0 (centre tap), conv_up1 reads feature 0 one pixel to the LEFT (tap ky 1, kx 0) with
    weight 2, conv_up2 and conv_hr copy feature 0, conv_last writes 0.5 x feature 0 + 0.25 into G.  The dense blocks then add nothing, conv_body adds nothing, so
    out[G][y][x] = 0.5 * 2 * E[y][x - 1] + 0.25 with E the source's R enlarged 4x and shifted (zero at column 0), exactly, in both evaluations"""
    w = {k: np.zeros_like(v) for k, v in R.random_weights(4, 1, 0).items()}
    w["conv_first.weight"][0, 0, 1, 1] = 1
    w["conv_up1.weight"][0, 0, 1, 0] = 2
    for n in ("conv_up2", "conv_hr"):
        w[n + ".weight"][0, 0, 1, 1] = 1
    w["conv_last.weight"][1, 0, 1, 1] = 0.5
    w["conv_last.bias"][1] = 0.25
    src = np.zeros((3, 4, 5), np.float16)
    src[0] = np.arange(20).reshape(4, 5) / 32.0
    up1 = np.zeros((8, 10))
    up1[:, 1:] = 2 * src[0].astype(np.float64).repeat(2, 0).repeat(2, 1)[:, :-1]
    want = 0.5 * up1.repeat(2, 0).repeat(2, 1) + 0.25
    for mode in ("M64", "Mh"):
        out = R.Model(w, 4, 1, mode)(src)
        assert out.shape == (3, 16, 20) and np.array_equal(out[1], want), mode
        assert not out[0].any() and not out[2].any()


def test_model_rounds_where_the_definition_rounds():
    """Mh differs from M64 (it rounds) by an error of the size of half precision, not more; and a residual pair is applied before the one rounding: with a1 = 0.2
    the value v * 0.2 + x is rounded once (two roundings would differ on this input)"""
    import torch
    m64, mh, e_h = S.net_models(S.NET_CASES[0])
    assert m64.dtype == np.float64 and mh.dtype == np.float32 and 0 < e_h < 2.0 ** -6
    assert np.array_equal(mh, mh.astype(np.float16).astype(np.float32))
    m = R.Model({"c.weight": np.full((1, 1, 3, 3), 0, np.float32), "c.bias": np.array([1 + 2.0 ** -12], np.float32)}, 4, 1, "Mh")
    x = torch.zeros((1, 2, 2))
    r = torch.full((1, 2, 2), 2.0 ** -11)
    once = m.conv("c", x, False, [(1.0, r)])
    assert float(once[0, 0, 0]) == float(np.float16(1 + 2.0 ** -12 + 2.0 ** -11)) == 1 + 2.0 ** -10 != float(np.float16(np.float16(1 + 2.0 ** -12) + np.float16(2.0 ** -11)))


# ------------------------------------------------------------------------------------------------ 2. the host side
def test_half_rounding_of_the_packer_is_numpys(emu):
    emu.emu_sr_half.argtypes = [C.c_float]
    emu.emu_sr_half.restype = C.c_uint
    rng = np.random.default_rng(5)
    vals = np.concatenate([rng.standard_normal(2000).astype(np.float32) * s for s in (1e-8, 1e-5, 1e-3, 1.0, 300.0, 70000.0)]
                          + [np.array([0.0, -0.0, 65504.0, 65519.9, 65520.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 2.0 ** -14, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,
                                       np.inf, -np.inf], np.float32)])
    with np.errstate(over="ignore"):
        want = vals.astype(np.float16).view(np.uint16)
    got = np.array([emu.emu_sr_half(float(v)) for v in vals], np.uint16)
    assert np.array_equal(got, want), vals[got != want][:5]


def test_counts_memory_and_launches(emu):
    count, nbytes, launches = C.c_ulonglong(), C.c_ulonglong(), C.c_int()
    for scale, blocks in ((4, 1), (2, 1), (4, 23), (2, 6)):
        assert emu.emu_sr_net_info(scale, blocks, 64, 48, C.byref(count), C.byref(nbytes), C.byref(launches)) == 0
        shapes = [R.layer_shape(n, scale) for n in R.layer_names(blocks)]
        assert count.value == sum(co * ci * 9 + co for co, ci in shapes) == R.flatten(R.random_weights(scale, blocks, 1), blocks).size
        t = 64 * 48 // (4 if scale == 2 else 1)
        per_pixel = 2 * (32 + 64 + 3 * 192 + 4 * 64 + 16 * 64 * 2 + 16 * 3)          # the formula of sr_net.h: 6048 bytes a pixel of the input tensor
        assert per_pixel == 6048 and per_pixel * t <= nbytes.value <= per_pixel * t + 9 * 256
        assert launches.value == len(shapes) + 1                                      # conv_first runs twice
    # the network of the reference's x4plus at 960x540: 3.1 GB
    assert emu.emu_sr_net_info(4, 23, 960, 540, C.byref(count), C.byref(nbytes), C.byref(launches)) == 0 and 3.1e9 < nbytes.value < 3.2e9
    assert emu.emu_sr_net_info(3, 1, 64, 48, C.byref(count), C.byref(nbytes), C.byref(launches)) == -3
    assert emu.emu_sr_net_info(2, 1, 63, 48, C.byref(count), C.byref(nbytes), C.byref(launches)) == 0 and nbytes.value == 0      # odd with scale 2


def test_packed_layout_is_the_documented_one(emu):
    """element j of lane l of fragment n of step (tap, chunk) is W[16 n + (l & 15)][32 chunk + 8 (l >> 4) + j][tap / 3][tap % 3], rounded to half; padding is zero"""
    rng = np.random.default_rng(3)
    for cout, cin, cout_pad, cin_pad in ((64, 12, 64, 32), (32, 96, 32, 96), (3, 64, 16, 64)):
        w = rng.standard_normal((cout, cin, 3, 3)).astype(np.float32)
        dst = np.full(9 * cin_pad * cout_pad, 0xFFFF, np.uint16)
        emu.emu_sr_pack.restype = None
        emu.emu_sr_pack(util.ptr(w), cout, cin, cout_pad, cin_pad, util.ptr(dst))
        wp = np.zeros((cout_pad, cin_pad, 3, 3), np.float16)
        wp[:cout, :cin] = w.astype(np.float16)
        d = dst.view(np.float16).reshape(9, cin_pad // 32, cout_pad // 16, 4, 16, 8)      # tap, chunk, n, l >> 4, l & 15, j
        want = wp.reshape(cout_pad // 16, 16, cin_pad // 32, 4, 8, 9).transpose(5, 2, 0, 3, 1, 4)
        assert np.array_equal(d.view(np.uint16), np.ascontiguousarray(want).view(np.uint16))


# ------------------------------------------------------------------------------------------------ 3. the stepped convolution, exactly
def test_tile_is_the_one_the_cases_are_built_around(emu):
    v = [C.c_int() for _ in range(4)]
    emu.emu_sr_tile(*map(C.byref, v))
    assert [x.value for x in v] == [S.TW, S.TH, 32, 16]


@pytest.mark.parametrize("case_id", S.CONV_IDS)
def test_stepped_conv_is_exact(emu, case_id):
    """the slice the launch writes equals the integer convolution bit for bit; everything else in the output buffer (neighbouring slices, garbage) is as it was"""
    out, want = S.run_conv(emu, "emu_", case_id, order=S.CONV_IDS.index(case_id) % 3, seed=7)
    assert np.array_equal(out, want), np.argwhere(out != want)[:5]


def test_exact_cases_reach_what_they_exist_for():
    """negative sums under the activation, sums that need the full range, residuals that change the value"""
    d, x, wt, bias, r1, r2, garbage, want = S.conv_data("conv5-17x33")
    assert d.n_res == 2 and d.cin == 192
    v = want[:, :, :64].view(np.float16).astype(np.float64)
    assert v.min() < -50 and v.max() > 50 and np.any(v != np.round(v))
    d1 = S.conv_data("feat-epilogue1")
    acc = R.conv_exact(d1[1].view(np.float16), d1[2], d1[3])
    assert (acc.astype(np.float64) < 0).mean() > 0.2


@pytest.mark.parametrize("order", [0, 1, 2])
def test_stepped_conv_in_every_thread_order_and_lds_image(emu, order):
    for case_id in ("conv5-17x9", "feat-up-5x7", "last-17x9"):
        out, want = S.run_conv(emu, "emu_", case_id, order=order, seed=100 + order)
        assert np.array_equal(out, want), case_id


# ------------------------------------------------------------------------------------------------ 4. the stepped input kernel
@pytest.mark.parametrize("scale", [4, 2])
@pytest.mark.parametrize("name", S.INPUT_FORMATS)
def test_stepped_input_is_numpys(emu, name, scale):
    want = S.input_want(name, scale)
    for order, align in ((0, 16), (2, 1)):
        assert np.array_equal(S.run_input(emu, "emu_", name, scale, order=order, align=align), want), (order, align)
    assert not want[:, :, 12 if scale == 2 else 3:].any() and want[:, :, :3].any()


# ------------------------------------------------------------------------------------------------ 5. the whole network, stepped
@pytest.mark.parametrize("case", S.NET_CASES, ids=S.net_id)
def test_half_model_error_is_finite_and_not_zero(case):
    m64, mh, e_h = S.net_models(case)
    assert np.isfinite(m64).all() and np.isfinite(mh).all() and 0 < e_h < 2.0 ** -6, e_h
    assert m64.shape == (3, case[2][1] * case[1], case[2][0] * case[1]) and np.ptp(m64) > (0.01 if case[3] == 0.1 else 2.0)


@pytest.mark.parametrize("case", S.STRONG_CASES, ids=S.net_id)
def test_the_bound_sees_every_part_of_the_network(case):
    """with plain Kaiming weights a network whose trunk is left out, whose first layer, conv4s, conv_body or enlarging layers are dead, or whose first two dense
    blocks are exchanged lies more than 4 bounds from M64.  A run with such a defect is at least d - bound from M64 when the same run without it is within the
    bound, so d > 2 bounds already fails the assertion; 4 is twice that.  (With the 0.1 weights a trunk left out stays inside the bound: those cases do not see
    it, which the last line holds on to.)"""
    _, _, e_h = S.net_models(case)
    bound = 2 * e_h + 2.0 ** -11
    for name, d in S.broken_networks(case).items():
        print(f"{S.net_id(case)} {name}: {d:.3e} = {d / bound:.0f} bounds")
        assert d > 4 * bound, name
    weak = S.NET_CASES[S.STRONG_CASES.index(case)]
    assert S.broken_networks(weak)["trunk left out"] < 2 * S.net_models(weak)[2] + 2.0 ** -11


@pytest.mark.parametrize("case", S.NET_CASES, ids=S.net_id)
def test_stepped_network_is_within_twice_the_half_models_error(emu, case):
    dev = S.run_network(emu, "emu_", case, order=S.NET_CASES.index(case) % 3)
    e_h, e_dev, bound = S.network_errors(dev, case)
    print(f"{S.net_id(case)}: E_h {e_h:.3e}  E_stepped {e_dev:.3e}  bound {bound:.3e}")
    assert e_dev <= bound


# ------------------------------------------------------------------------------------------------ 6. sanitizers
def test_stepped_kernels_under_address_sanitizer(tmp_path):
    """a stand-alone program (its own main, no python in the process): the packer, the launch list and both stepped kernels over tensors and planes that end with
    their last element.  A read or write past one ends it with the sanitizer's report"""
    exe = tmp_path / "sr_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w", "-o", str(exe),
                    str(ROOT / "tests" / "emu" / "sr.cpp"), str(ROOT / "tests" / "sr_asan_main.cc")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("runs")


# ------------------------------------------------------------------------------------------------ 7. the entries without a device
def test_stage_entries_validate_first():
    lib = _lib.load()
    d, x, wt, bias, r1, r2, garbage, _ = S.conv_data("conv1-4x4")
    out = garbage.copy()
    args = [util.ptr(a) for a in (x, wt, bias, r1, r2, out)]
    no_device = _lib.ENODEV if lib.mihevc_device_count() == 0 else 0
    assert lib.mihevc_k_sr_conv(0, C.byref(d), *args) == no_device
    for field, value in (("cin", 48), ("cin", 224), ("cout", 48), ("in_off", 4), ("out_off", 176), ("n_res", 3), ("width", 0), ("up", 2), ("cin_real", 65)):
        bad = _lib.SrConvDesc.from_buffer_copy(bytes(d))
        setattr(bad, field, value)
        assert lib.mihevc_k_sr_conv(0, C.byref(bad), *args) == _lib.EINVAL, field
    assert lib.mihevc_k_sr_conv(0, C.byref(d), None, *args[1:]) == _lib.EINVAL
    planar = _lib.SrConvDesc.from_buffer_copy(bytes(S.conv_data("last-17x9")[0]))
    planar.n_res, planar.r1_ch = 1, 64                                                  # the last layer takes no residual
    assert lib.mihevc_k_sr_conv(0, C.byref(planar), *args) == _lib.EINVAL
    fmt = _lib.rgb_format_for("gbrp")
    planes, _ = S.net_source((12, 20))
    _, flat = S.net_weights(1, 4)
    o = np.zeros((3, 80, 48), np.uint16)
    p = [util.ptr(a) for a in planes]
    call = lambda model, count=flat.size, w=12, h=20, f=fmt: lib.mihevc_k_sr_network(0, C.byref(model), util.ptr(flat), count, C.byref(f), w, h, *p, w, util.ptr(o))
    assert call(_lib.SrModel(4, 1)) == no_device
    assert call(_lib.SrModel(3, 1)) == call(_lib.SrModel(4, 0)) == call(_lib.SrModel(4, 1), count=flat.size - 1) == call(_lib.SrModel(2, 1)) == _lib.EINVAL
    assert call(_lib.SrModel(4, 1), w=3) == _lib.EINVAL
    bad_model = _lib.SrModel(4, 1)
    bad_model.reserved[2] = 1
    assert call(bad_model) == _lib.EINVAL
    assert lib.mihevc_k_sr_input(0, C.byref(fmt), 2, 13, 20, *p, 13, util.ptr(o)) == _lib.EINVAL          # odd with scale 2
    assert lib.mihevc_k_sr_input(0, C.byref(fmt), 4, 12, 20, *p, 11, util.ptr(o)) == _lib.EINVAL          # a pitch below the row
