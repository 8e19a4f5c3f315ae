"""What the tests of the learned super-resolution path share (test_sr_cpu, test_gpu_sr and its child process sr_device_child): the cases of the exact
convolution tests with their inputs and integer references, the sources and formats of the input-kernel tests, the networks of the whole-network tests with
their two model evaluations, all computed once, and the ctypes calls, which are the same for the stepped library (emu_) and the device (mihevc_k_)."""
import ctypes as C
import functools

import numpy as np

from hevc_amd import _lib
from tests import sr_ref as R
from tests import util

TW, TH = 16, 8          # the kernel's tile; test_sr_cpu checks it against emu_sr_tile
SLOPE_EXACT = 0.25      # the exact tests pass an exact slope through the stage entry (0.2 is not a dyadic fraction); the network tests run the real 0.2

# (name, cin, cin_real, in_ch, cout, out_ch, out_off, planar): the shapes of the network, written into the slices a network writes them to
CHANNELS = [
    ("first4", 32, 3, 32, 64, 64, 0, 0), ("first2", 32, 12, 32, 64, 192, 0, 0), ("conv1", 64, 64, 192, 32, 192, 64, 0), ("conv2", 96, 96, 192, 32, 192, 96, 0),
    ("conv3", 128, 128, 192, 32, 192, 128, 0), ("conv4", 160, 160, 192, 32, 192, 160, 0), ("conv5", 192, 192, 192, 64, 192, 0, 0),
    ("feat", 64, 64, 64, 64, 64, 0, 0), ("last", 64, 64, 64, 3, 3, 0, 1),
]
# 4x4; one pixel less, exactly one and one pixel more than a tile per axis; several tiles with a remainder each way
SIZES = [(4, 4), (TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (17, 33), (40, 24)]
# (act, n_res, a1, a2)
EPILOGUES = [(0, 0, 1.0, 1.0), (1, 0, 1.0, 1.0), (0, 1, 0.5, 1.0), (1, 1, 1.0, 1.0), (0, 2, 0.5, 0.5), (1, 2, 0.5, 1.0)]
UP_SOURCES = [(5, 7), (9, 4)]


def conv_cases():
    """(id, channels entry, (w, h), up, epilogue): every channel shape at a size of 2 x 2 tiles, every size at a slice-writing shape and at the widest one,
    every epilogue, the folded enlargement"""
    out = []
    for ch in CHANNELS:
        out.append((f"{ch[0]}-17x9", ch, (17, 9), 0, EPILOGUES[1] if not ch[7] else EPILOGUES[0]))
    for w, h in SIZES:
        out.append((f"conv1-{w}x{h}", CHANNELS[2], (w, h), 0, EPILOGUES[1]))
        out.append((f"conv5-{w}x{h}", CHANNELS[6], (w, h), 0, EPILOGUES[4]))
    for i, e in enumerate(EPILOGUES):
        out.append((f"feat-epilogue{i}", CHANNELS[7], (19, 10), 0, e))
    for sw, sh in UP_SOURCES:
        out.append((f"feat-up-{sw}x{sh}", CHANNELS[7], (2 * sw, 2 * sh), 1, EPILOGUES[1]))
        out.append((f"last-up-{sw}x{sh}", CHANNELS[8], (2 * sw, 2 * sh), 1, EPILOGUES[0]))
    return out


CONV_CASES = conv_cases()
CONV_IDS = [c[0] for c in CONV_CASES]


def half_bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float16)).view(np.uint16)


@functools.lru_cache(maxsize=None)
def conv_data(case_id):
    """the arrays of a case, made once: descriptor fields, input buffer, weights, bias, residual buffers, the garbage-filled output buffer and the expected one"""
    _, (name, cin, cin_real, in_ch, cout, out_ch, out_off, planar), (w, h), up, (act, n_res, a1, a2) = CONV_CASES[CONV_IDS.index(case_id)]
    rng = np.random.default_rng(sum(map(ord, case_id)) * 7919)
    sw, sh = ((w + 1) // 2, (h + 1) // 2) if up else (w, h)
    x = rng.integers(-1, 2, (sh, sw, in_ch)).astype(np.float16)              # every channel of the buffer, those the launch does not read included
    wt = rng.integers(-1, 2, (cout, cin_real, 3, 3)).astype(np.float32)
    bias = rng.integers(-256, 257, cout).astype(np.float32)
    r1_ch, r1_off, r2_ch, r2_off = (192, 0, 64, 0) if cout == 64 else (64, 32, 64, 0)
    r1 = rng.integers(-8, 9, (h, w, r1_ch)).astype(np.float16)
    r2 = rng.integers(-8, 9, (h, w, r2_ch)).astype(np.float16)
    res = [(a1, r1[:, :, r1_off:r1_off + cout]), (a2, r2[:, :, r2_off:r2_off + cout])][:n_res]
    want_slice = R.conv_exact(x[:, :, :cin_real], wt, bias, up=bool(up), act=bool(act), slope=SLOPE_EXACT, res=res)
    garbage = rng.integers(0, 1 << 16, (3, h, w) if planar else (h, w, out_ch)).astype(np.uint16)
    want = garbage.copy()
    if planar:
        want[:] = half_bits(want_slice).transpose(2, 0, 1)
    else:
        want[:, :, out_off:out_off + cout] = half_bits(want_slice)
    d = _lib.SrConvDesc(w, h, up, planar, act, n_res, in_ch, 0, cin, cin_real, out_ch, out_off, cout, r1_ch, r1_off, r2_ch, r2_off, SLOPE_EXACT, a1, a2)
    return d, half_bits(x), wt, bias, half_bits(r1), half_bits(r2), garbage, want


def run_conv(lib, prefix, case_id, device=None, order=0, seed=1):
    """the output buffer after one launch, and the expected one"""
    d, x, wt, bias, r1, r2, garbage, want = conv_data(case_id)
    out = garbage.copy()
    args = [C.byref(d), util.ptr(x), util.ptr(wt), util.ptr(bias), util.ptr(r1), util.ptr(r2), util.ptr(out)]
    if prefix == "emu_":
        lib.emu_sr_conv.argtypes = [C.POINTER(_lib.SrConvDesc)] + [C.c_void_p] * 6 + [C.c_int, C.c_uint]
        rc = lib.emu_sr_conv(*args, order, seed)
    else:
        rc = lib.mihevc_k_sr_conv(device, *args)
    assert rc == 0, rc
    return out, want


# ------------------------------------------------------------------------------------------------ the input kernel
INPUT_FORMATS = ["gbrp", "rgb24", "bgra", "gbrp10le", "gbrpf32le", "gbrpf16"]       # gbrpf16: half planes, which ffmpeg has no name for (sample = 1)
INPUT_SIZE = (22, 14)


def input_format(name):
    return _lib.RgbFormat(0, 2, 0, 1, 1, 0, 0, 0) if name == "gbrpf16" else _lib.rgb_format_for(name)


@functools.lru_cache(maxsize=None)
def input_data(name):
    """(format, the source planes as the entry takes them, [3, H, W] R G B values, peak or None)"""
    fmt = input_format(name)
    w, h = INPUT_SIZE
    rng = np.random.default_rng(len(name) * 131 + sum(map(ord, name)))
    if fmt.sample:
        rgb = rng.uniform(-0.1, 1.1, (3, h, w)).astype(np.float32 if fmt.sample == 2 else np.float16)
        rgb[0, 0, 0] = np.nan
        rgb[1, 0, 1] = 1.0
        peak = None
    else:
        dt = np.uint16 if fmt.bit_depth > 8 else np.uint8
        rgb = rng.integers(0, np.iinfo(dt).max + 1, (3, h, w)).astype(dt)        # 10 bit: values above the depth too
        rgb[0, 0, 0], rgb[1, 0, 1] = 0, (1 << fmt.bit_depth) - 1
        peak = (1 << fmt.bit_depth) - 1
    if fmt.layout == 0:
        planes = [None] * 3
        for c, pos in enumerate((fmt.r, fmt.g, fmt.b)):
            planes[pos] = np.ascontiguousarray(rgb[c])
    else:
        packed = rng.integers(0, 256, (h, w, fmt.layout)).astype(rgb.dtype)
        for c, pos in enumerate((fmt.r, fmt.g, fmt.b)):
            packed[:, :, pos] = rgb[c]
        planes = [np.ascontiguousarray(packed.reshape(h, w * fmt.layout))]
    return fmt, planes, rgb, peak


def input_want(name, scale):
    """the input tensor [th, tw, 32] as half bits"""
    import torch
    _, _, rgb, peak = input_data(name)
    x = R.input_tensor(list(rgb), peak)
    if scale == 2:
        x = R.pixel_unshuffle(torch.from_numpy(x.astype(np.float32))).numpy().astype(np.float16)
    out = np.zeros(x.shape[1:] + (32,), np.float16)
    out[:, :, :x.shape[0]] = x.transpose(1, 2, 0)
    return half_bits(out)


def run_input(lib, prefix, name, scale, device=None, order=0, align=16):
    fmt, planes, _, _ = input_data(name)
    w, h = INPUT_SIZE
    f = 2 if scale == 2 else 1
    out = np.full((h // f, w // f, 32), 0xA5A5, np.uint16)
    p = [util.ptr(planes[i]) if i < len(planes) else None for i in range(3)]
    if prefix == "emu_":
        lib.emu_sr_input.argtypes = [C.POINTER(_lib.RgbFormat), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        rc = lib.emu_sr_input(C.byref(fmt), scale, w, h, *p, align, util.ptr(out), order)
    else:
        rc = lib.mihevc_k_sr_input(device, C.byref(fmt), scale, w, h, *p, planes[0].shape[1], util.ptr(out))
    assert rc == 0, rc
    return out


# ------------------------------------------------------------------------------------------------ the whole network
# (blocks, scale, (source width, height), gain).  Gain 0.1: the weights the network's initialisation has (Kaiming x 0.1), B = 1 and 2, both scales, both sizes.
# With them a layer passes on about a seventh of what it receives, and everything in front of conv_hr reaches the output below half precision: those cases hold
# the last layers and the plumbing, and cannot see the trunk.  Gain 1 (plain Kaiming, the last four cases) keeps every layer's share of the output far above the
# bound; test_sr_cpu shows that a trunk left out, a dead first layer, two dense blocks exchanged, a dead conv4 or a dead conv_body each move M64 by more than 4
# times the bound there (7 to 700 times, measured).  The stepped run and the device run take the same twelve cases.
_SHAPES = [(1, 4, (12, 20)), (2, 4, (22, 14)), (1, 2, (22, 14)), (2, 2, (12, 20)), (2, 4, (12, 20)), (1, 4, (22, 14)), (2, 2, (22, 14)), (1, 2, (12, 20))]
NET_CASES = [c + (0.1,) for c in _SHAPES] + [c + (1.0,) for c in _SHAPES[:4]]
STRONG_CASES = NET_CASES[8:]


def net_id(c):
    return f"B{c[0]}-x{c[1]}-{c[2][0]}x{c[2][1]}" + ("" if c[3] == 0.1 else "-kaiming")


@functools.lru_cache(maxsize=None)
def net_weights(blocks, scale, gain=0.1):
    w = R.random_weights(scale, blocks, 1000 * blocks + scale, gain)
    return w, R.flatten(w, blocks)


@functools.lru_cache(maxsize=None)
def net_source(size):
    """gbrp, 8 bit: planes in G, B, R order, and the [3, H, W] R G B array"""
    w, h = size
    rng = np.random.default_rng(w * 100 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    rgb = np.stack([(128 + 100 * np.sin(xx / (2.0 + c) + yy / 3.0) + rng.integers(-20, 21, (h, w))).clip(0, 255) for c in range(3)]).astype(np.uint8)
    return [np.ascontiguousarray(rgb[1]), np.ascontiguousarray(rgb[2]), np.ascontiguousarray(rgb[0])], rgb


@functools.lru_cache(maxsize=None)
def net_models(case):
    """(M64 output, Mh output, E_h) of a case"""
    blocks, scale, size, gain = case
    w, _ = net_weights(blocks, scale, gain)
    x = R.input_tensor(list(net_source(size)[1]), 255)
    m64 = R.Model(w, scale, blocks, "M64")(x)
    mh = R.Model(w, scale, blocks, "Mh")(x)
    return m64, mh, float(np.max(np.abs(mh.astype(np.float64) - m64)))


def broken_networks(case):
    """name -> max |M64 of a network with one defect - M64|: what a launch list that dropped or mis-wired that part would compute"""
    blocks, scale, size, gain = case
    w, _ = net_weights(blocks, scale, gain)
    x = R.input_tensor(list(net_source(size)[1]), 255)
    m64 = net_models(case)[0]

    def zero(pred):
        return {k: (np.zeros_like(v) if pred(k) else v) for k, v in w.items()}

    swapped = dict(w)
    for k in range(1, 6):
        for sfx in (".weight", ".bias"):
            swapped[f"body.0.rdb1.conv{k}{sfx}"], swapped[f"body.0.rdb2.conv{k}{sfx}"] = w[f"body.0.rdb2.conv{k}{sfx}"], w[f"body.0.rdb1.conv{k}{sfx}"]
    variants = {"trunk left out": zero(lambda k: k.startswith("body.")), "conv_first dead": zero(lambda k: k == "conv_first.weight"), "rdb1 and rdb2 exchanged": swapped,
                "every conv4 dead": zero(lambda k: k.endswith("conv4.weight")), "conv_body dead": zero(lambda k: k == "conv_body.weight"),
                "conv_up1 dead": zero(lambda k: k == "conv_up1.weight"), "conv_up2 dead": zero(lambda k: k == "conv_up2.weight")}
    return {n: float(np.max(np.abs(R.Model(v, scale, blocks, "M64")(x) - m64))) for n, v in variants.items()}


def run_network(lib, prefix, case, device=None, order=0, seed=1):
    """[3, scale H, scale W] float16"""
    blocks, scale, (w, h), gain = case
    _, flat = net_weights(blocks, scale, gain)
    planes, _ = net_source((w, h))
    fmt = _lib.rgb_format_for("gbrp")
    model = _lib.SrModel(scale, blocks)
    out = np.zeros((3, h * scale, w * scale), np.uint16)
    head = [C.byref(model), util.ptr(flat), flat.size, C.byref(fmt), w, h, *map(util.ptr, planes)]
    if prefix == "emu_":
        lib.emu_sr_network.argtypes = [C.POINTER(_lib.SrModel), C.c_void_p, C.c_size_t, C.POINTER(_lib.RgbFormat), C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_uint]
        rc = lib.emu_sr_network(*head, util.ptr(out), order, seed)
    else:
        rc = lib.mihevc_k_sr_network(device, *head, w, util.ptr(out))
    assert rc == 0, rc
    return out.view(np.float16)


def network_errors(dev, case):
    """(E_h, E_dev, bound): over every output element"""
    m64, _, e_h = net_models(case)
    e_dev = float(np.max(np.abs(dev.astype(np.float64) - m64)))
    return e_h, e_dev, 2 * e_h + 2.0 ** -11


# ------------------------------------------------------------------------------------------------ GPU sessions: 48x32 (scale 4) or 96x64 (scale 2) to 192x128, B = 1
SESSION_W, SESSION_H, SESSION_N = 192, 128, 4
HALF_PLANES = (0, 0, 1, 2, 1, 0)          # RgbFormat: three planes of halves, R, G, B: what mihevc_k_sr_network returns


def session_cfg(depth):
    from tests.ingest_common import base_cfg
    cfg = base_cfg(depth)
    cfg.width, cfg.height, cfg.matrix = SESSION_W, SESSION_H, 1
    return cfg


@functools.lru_cache(maxsize=None)
def session_model(scale, seed=0):
    """hevc_amd.sr.RrdbNet: the gaussian weights, plus a path that carries the picture through (feature c = component c, copied by the centre taps), so that
    the output is the enlarged source with the network's texture on it and not a flat field"""
    from hevc_amd import sr
    w = R.random_weights(scale, 1, 77 + seed)
    for c in range(3):
        w["conv_first.weight"][c, c * 4 if scale == 2 else c, 1, 1] += 1.0
        for n in ("conv_up1", "conv_up2", "conv_hr"):
            w[n + ".weight"][c, c, 1, 1] += 1.0
        w["conv_last.weight"][c, c, 1, 1] += 1.0 - 0.25 * seed
    return sr.RrdbNet(scale, 1, R.flatten(w, 1))


@functools.lru_cache(maxsize=None)
def session_clip(scale, depth):
    """SESSION_N pictures of a moving scene as gbrp (8 bit) or gbrp10le planes in G, B, R order"""
    sw, sh = SESSION_W // scale, SESSION_H // scale
    out = []
    for i in range(SESSION_N):
        f = util.synth_frame(max(sh, 40), max(sw, 48), seed=9, shift=(3 * i, 2 * i), bit_depth=depth)
        y = np.asarray(f.y)[:sh, :sw].astype(np.uint16 if depth > 8 else np.uint8)
        out.append([np.ascontiguousarray(y), np.ascontiguousarray(y[::-1]), np.ascontiguousarray(y[:, ::-1])])
    return out


def session_format(depth):
    return _lib.rgb_format_for("gbrp10le" if depth > 8 else "gbrp")


def network_planes(lib, model, fmt, planes):
    """the three half planes mihevc_k_sr_network returns for a source: uint16 views, [3, H, W]"""
    h, w = planes[0].shape
    out = np.zeros((3, h * model.scale, w * model.scale), np.uint16)
    m = _lib.SrModel(model.scale, model.blocks)
    rc = lib.mihevc_k_sr_network(0, C.byref(m), util.ptr(model.weights), model.weights.size, C.byref(fmt), w, h, *map(util.ptr, planes), w, util.ptr(out))
    assert rc == 0, rc
    return out
