"""What the tests of the compact super-resolution path share (test_sr_compact_cpu, test_gpu_sr_compact): the cases of the exact convolution tests with their
inputs and integer references, the networks of the whole-network tests with their two model evaluations and their defective variants, all computed once, the
session models and clips, and the ctypes calls, which are the same for the stepped library (emu_) and the device (mihevc_k_)."""
import ctypes as C
import functools

import numpy as np

from hevc_amd import _lib
from tests import sr_compact_ref as R
from tests import sr_common as S
from tests import util

TW, TH = 16, 16          # the kernel's tile; test_sr_compact_cpu checks it against emu_sr_compact_tile
SLOPES_EXACT = (-0.5, 0.0, 0.25, 0.5, 1.0)

# name -> (cin, cin_real, tail, scale)
SHAPES = {"first": (32, 3, 0, 0), "trunk": (64, 64, 0, 0), "tail4": (64, 64, 1, 4), "tail2": (64, 64, 1, 2)}
# 4x4; one pixel less, exactly one and one pixel more than a tile per axis; several tiles with a remainder each way (3 x 3 tiles)
SIZES = [(4, 4), (TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (37, 35)]
# more tiles than a launch has workgroups (17 x 17 = 289 > 256): workgroups walk a second tile.  The device runs it; the stepped runs reach the same loop
# through fewer workgroups (test_sr_compact_cpu test_fewer_workgroups_walk_the_same_tiles), since stepping 289 tiles takes a minute
MANY_TILES = "trunk-265x261"


def conv_cases():
    out = [(f"{name}-{w}x{h}", name, (w, h)) for name in SHAPES for w, h in SIZES]
    return out + [(MANY_TILES, "trunk", (265, 261))]


CONV_CASES = conv_cases()
CONV_IDS = [c[0] for c in CONV_CASES]
STEPPED_IDS = [i for i in CONV_IDS if i != MANY_TILES]
half_bits = S.half_bits


@functools.lru_cache(maxsize=None)
def conv_data(case_id):
    """the arrays of a case, made once: (descriptor, input, weights, bias, slopes or None, base or None, the garbage-filled output buffer, the expected one, facts);
    facts: what the case reaches (see test_the_exact_cases_reach_what_they_exist_for)"""
    _, name, (w, h) = CONV_CASES[CONV_IDS.index(case_id)]
    cin, cin_real, tail, scale = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, case_id)) * 7919 + 5)
    x = rng.integers(-1, 2, (h, w, cin)).astype(np.float16)              # every channel of the tensor, those that meet zero weights included
    d = _lib.SrCompactConvDesc(w, h, cin, cin_real, tail, scale)
    if not tail:
        wt = rng.integers(-1, 2, (64, cin_real, 3, 3)).astype(np.float32)
        bias = rng.integers(-8 if cin_real == 3 else -64, 9 if cin_real == 3 else 65, 64).astype(np.float32)
        slopes = rng.choice(np.array(SLOPES_EXACT, np.float32), 64)
        want, sums = R.conv_prelu_exact(x[:, :, :cin_real], wt, bias, slopes)
        facts = {"negative under a slope": int(((sums < 0) & ~np.isin(slopes, (0.0, 1.0))[None, None, :]).sum()),
                 "pixels with different slopes": int((np.where(sums < 0, slopes[None, None, :], -np.inf).max(axis=2) > np.where(sums < 0, slopes[None, None, :], np.inf).min(axis=2)).sum())}
        garbage = rng.integers(0, 1 << 16, (h, w, 64)).astype(np.uint16)
        return d, half_bits(x), wt, bias, slopes, None, garbage, half_bits(want), facts
    r = scale
    wt = rng.integers(-1, 2, (3 * r * r, 64, 3, 3)).astype(np.float32)
    bias = rng.integers(-8, 9, 3 * r * r).astype(np.float32)
    base = np.zeros((h, w, 32), np.float16)
    base[:, :, :3] = rng.integers(0, 257, (h, w, 3)) / 256.0
    base[:, :, 3:] = rng.integers(-1, 2, (h, w, 29))                     # (channels the tail must not read)
    want, without = R.conv_tail_exact(x, wt, bias, base[:, :, :3], r)
    facts = {"base changes the half": int((half_bits(want) != half_bits(without)).sum())}
    garbage = rng.integers(0, 1 << 16, (3, r * h, r * w)).astype(np.uint16)
    return d, half_bits(x), wt, bias, None, half_bits(base), garbage, half_bits(want), facts


def run_conv(lib, prefix, case_id, device=None, order=0, seed=1, nwg=0):
    """the output buffer after one launch, and the expected one"""
    d, x, wt, bias, slopes, base, garbage, want, _ = conv_data(case_id)
    out = garbage.copy()
    args = [C.byref(d), util.ptr(x), util.ptr(wt), util.ptr(bias), None if slopes is None else util.ptr(slopes), None if base is None else util.ptr(base), util.ptr(out)]
    if prefix == "emu_":
        lib.emu_sr_compact_conv.argtypes = [C.POINTER(_lib.SrCompactConvDesc)] + [C.c_void_p] * 6 + [C.c_int, C.c_uint, C.c_int]
        rc = lib.emu_sr_compact_conv(*args, order, seed, nwg)
    else:
        rc = lib.mihevc_k_sr_compact_conv(device, *args)
    assert rc == 0, rc
    return out, want


# ------------------------------------------------------------------------------------------------ the whole network
# (convs, scale, (source width, height)).  Plain Kaiming weights (gain 1) and slopes uniform in [-0.2, 0.6] per channel: every layer's share of the output
# stays far above the bound, so the bound sees every defect of broken_networks (test_sr_compact_cpu test_the_bound_sees_every_defect)
NET_CASES = [(convs, scale, size) for convs in (1, 2, 3) for scale, size in ((4, (12, 20)), (4, (22, 14)), (2, (12, 20)), (2, (22, 14)), (2, (13, 21)))]


def net_id(c):
    return f"C{c[0]}-x{c[1]}-{c[2][0]}x{c[2][1]}"


@functools.lru_cache(maxsize=None)
def net_weights(convs, scale):
    w = R.random_weights(scale, convs, 2000 * convs + scale)
    return w, R.flatten(w, convs)


@functools.lru_cache(maxsize=None)
def net_source(size):
    """gbrp, 8 bit: planes in G, B, R order, and the [3, H, W] R G B array (odd sizes too)"""
    w, h = size
    rng = np.random.default_rng(w * 100 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    rgb = np.stack([(128 + 100 * np.sin(xx / (2.0 + c) + yy / 3.0) + rng.integers(-20, 21, (h, w))).clip(0, 255) for c in range(3)]).astype(np.uint8)
    return [np.ascontiguousarray(rgb[1]), np.ascontiguousarray(rgb[2]), np.ascontiguousarray(rgb[0])], rgb


def _input(size):
    from tests import sr_ref
    return sr_ref.input_tensor(list(net_source(size)[1]), 255)


@functools.lru_cache(maxsize=None)
def net_models(case):
    """(M64 output, Mh output, E_h) of a case"""
    convs, scale, size = case
    w, _ = net_weights(convs, scale)
    x = _input(size)
    m64 = R.Model(w, scale, convs, "M64")(x)
    mh = R.Model(w, scale, convs, "Mh")(x)
    return m64, mh, float(np.max(np.abs(mh.astype(np.float64) - m64)))


def broken_networks(case):
    """name -> max |M64 of a network with one defect - M64|: what a launch list, a packer or an epilogue with that defect would compute"""
    convs, scale, size = case
    w, _ = net_weights(convs, scale)
    x = _input(size)
    m64 = net_models(case)[0]
    r = scale
    last = 2 * convs + 2

    def trunk(i):
        return [f"body.{2 * i + 2}.weight", f"body.{2 * i + 2}.bias", f"body.{2 * i + 3}.weight"]

    left_out = {}          # trunk layer min(1, convs - 1) removed, the rest renumbered
    gone = min(1, convs - 1)
    for k, v in w.items():
        i = int(k.split(".")[1])
        if i // 2 - 1 == gone:
            continue
        left_out[k.replace(f"body.{i}.", f"body.{i - 2 if i // 2 - 1 > gone else i}.")] = v
    perm = np.arange(3 * r * r).reshape(3, r, r).transpose(0, 2, 1).reshape(-1)
    variants = {"a trunk layer left out": (left_out, convs - 1, {}),
                "slopes replaced by their mean": ({k: (np.full_like(v, v.mean()) if v.ndim == 1 and int(k.split(".")[1]) % 2 else v) for k, v in w.items()}, convs, {}),
                "slopes treated as 0": ({k: (np.zeros_like(v) if v.ndim == 1 and int(k.split(".")[1]) % 2 else v) for k, v in w.items()}, convs, {}),
                "dy and dx of the shuffle exchanged": ({k: (v[perm] if int(k.split(".")[1]) == last else v) for k, v in w.items()}, convs, {}),
                "the base add missing": (w, convs, {"base": False}),
                "the first layer dead": ({k: (np.zeros_like(v) if k == "body.0.weight" else v) for k, v in w.items()}, convs, {})}
    if convs == 3:
        sw = dict(w)
        for a, b in zip(trunk(1), trunk(2)):
            sw[a], sw[b] = w[b], w[a]
        variants["two trunk layers exchanged"] = (sw, convs, {})
    out = {}
    for n, (v, c, opt) in variants.items():
        m = R.Model(v, scale, c, "M64")
        y = m(x) if opt.get("base", True) else m(x) - np.repeat(np.repeat(np.asarray(x, np.float64), r, axis=1), r, axis=2)
        out[n] = float(np.max(np.abs(y - m64)))
    return out


def run_network(lib, prefix, case, device=None, order=0, seed=1):
    """[3, scale H, scale W] float16"""
    convs, scale, (w, h) = case
    _, flat = net_weights(convs, scale)
    planes, _ = net_source((w, h))
    fmt = _lib.rgb_format_for("gbrp")
    model = _lib.SrCompact(scale, convs)
    out = np.zeros((3, h * scale, w * scale), np.uint16)
    head = [C.byref(model), util.ptr(flat), flat.size, C.byref(fmt), w, h, *map(util.ptr, planes)]
    if prefix == "emu_":
        lib.emu_sr_compact_network.argtypes = [C.POINTER(_lib.SrCompact), C.c_void_p, C.c_size_t, C.POINTER(_lib.RgbFormat), C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_uint]
        rc = lib.emu_sr_compact_network(*head, util.ptr(out), order, seed)
    else:
        rc = lib.mihevc_k_sr_compact_network(device, *head, w, util.ptr(out))
    assert rc == 0, rc
    return out.view(np.float16)


def network_errors(dev, case):
    """(E_h, E_dev, bound): over every output element"""
    m64, _, e_h = net_models(case)
    e_dev = float(np.max(np.abs(dev.astype(np.float64) - m64)))
    return e_h, e_dev, 2 * e_h + 2.0 ** -11


# ------------------------------------------------------------------------------------------------ GPU sessions: 48x32 (scale 4) or 96x64 (scale 2) to 192x128
SESSION_CONVS = 2


@functools.lru_cache(maxsize=None)
def session_model(scale, seed=0):
    """hevc_amd.sr.CompactNet: gaussian weights at a third of Kaiming's deviation, plus a path that carries the picture through the layers (feature c =
    component c, copied by the centre taps, and added to every sample of its plane by the last layer), so that the output is the enlarged source with the
    network's texture on it and not a flat field"""
    from hevc_amd import sr
    w = R.random_weights(scale, SESSION_CONVS, 177 + seed, gain=0.3, tail_gain=0.1)
    r = scale
    for c in range(3):
        for i in range(SESSION_CONVS + 1):
            w[f"body.{2 * i}.weight"][c, c, 1, 1] += 1.0
        w[f"body.{2 * SESSION_CONVS + 2}.weight"][c * r * r:(c + 1) * r * r, c, 1, 1] += 0.25 * (seed - 1)
    return sr.CompactNet(scale, SESSION_CONVS, R.flatten(w, SESSION_CONVS))


def network_planes(lib, model, fmt, planes):
    """the three half planes mihevc_k_sr_compact_network returns for a source: uint16 views, [3, H, W]"""
    h, w = planes[0].shape
    out = np.zeros((3, h * model.scale, w * model.scale), np.uint16)
    m = _lib.SrCompact(model.scale, model.convs)
    rc = lib.mihevc_k_sr_compact_network(0, C.byref(m), util.ptr(model.weights), model.weights.size, C.byref(fmt), w, h, *map(util.ptr, planes), w, util.ptr(out))
    assert rc == 0, rc
    return out
