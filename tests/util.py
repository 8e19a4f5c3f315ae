"""Shared helpers of the test-suite: deterministic synthetic pictures and array plumbing between the oracle
(uint16 containers) and the product C ABI (uint8 planes at 8 bit, uint16 at 10 bit)."""
import collections
import ctypes as C
import functools
import os
import subprocess
from collections import namedtuple
from pathlib import Path

import numpy as np

from oracle import oracle as O
from tests import hevc_analysis as A

ROOT = Path(__file__).resolve().parents[1]
EMU_DIR = ROOT / "tests" / "emu"


def synth_frame(h, w, seed=0, shift=(0, 0), bit_depth=8, detail=True) -> O.Frame:
    """Band-limited texture + sine + moving rectangles + per-frame grain; `shift` translates the texture."""
    rng = np.random.default_rng(seed)
    big = rng.normal(0, 1, (h + 384, w + 384))          # room for shifts up to +-190 samples
    for _ in range(3):
        big = (big + np.roll(big, 1, 0) + np.roll(big, 1, 1) + np.roll(big, -1, 0) + np.roll(big, -1, 1)) / 5
    big = (big - big.min()) / (big.max() - big.min())
    oy, ox = 192 + shift[1], 192 + shift[0]
    y = big[oy:oy + h, ox:ox + w] * 180 + 30
    yy, xx = np.mgrid[0:h, 0:w]
    y = y + 15 * np.sin((xx + shift[0]) / 7.0)
    if detail:
        r2 = np.random.default_rng(seed + 7)
        for _ in range(max(2, (h * w) // 4096)):          # sharp-edged rectangles: force small CUs / angular modes
            rw, rh = int(r2.integers(4, 40)), int(r2.integers(4, 40))
            rx, ry = int(r2.integers(0, max(1, w - rw))), int(r2.integers(0, max(1, h - rh)))
            rx = (rx + shift[0] * 2) % max(1, w - rw)
            y[ry:ry + rh, rx:rx + rw] = r2.integers(16, 235)
        # a high-frequency checker patch
        y[h // 2:h // 2 + 16, 8:40] = np.where(((xx[:16, :32] // 2) + (yy[:16, :32] // 2)) % 2 == 0, 40, 210)
    g = np.random.default_rng((seed * 1000 + shift[0] * 31 + shift[1] + 1) % (1 << 32))      # negative shifts with seed 0: numpy takes non-negative seeds only
    y = np.clip(y + g.normal(0, 1.5, (h, w)), 0, 255)
    u = np.clip(128 + 30 * np.sin(yy[::2, ::2] / 9.0) + 20 * big[oy:oy + h:2, ox:ox + w:2] + g.normal(0, 1, (h // 2, w // 2)), 0, 255)
    v = np.clip(128 + 30 * np.cos(xx[::2, ::2] / 11.0) - 20 * big[oy:oy + h:2, ox:ox + w:2] + g.normal(0, 1, (h // 2, w // 2)), 0, 255)
    sc = 1 << (bit_depth - 8)
    return O.Frame((y * sc).astype(np.uint16), (u * sc).astype(np.uint16), (v * sc).astype(np.uint16))


ENVELOPE_KINDS = ("full_range", "rails")


def envelope_frame(kind, h, w, bit_depth=8, seed=0, shift=(0, 0)) -> O.Frame:
    """Content at the ends of the sample range, where synth_frame never goes (it stays mostly inside 15..240, x4 at 10 bit).
    'full_range': band-limited textures stretched past 0 and 2^bd - 1 and clipped, so that several per cent of every plane, chroma
    included, sit at each end (at 10 bit 1021..1023 occur too).  'rails': a mid-grey texture under hard-edged blocks of 0 and 2^bd - 1
    whose edges miss the 8x8 grid, plus black fields with single bright samples.  `shift` translates the content (P and B input) and
    changes only the per-picture grain, which never touches a rail."""
    assert kind in ENVELOPE_KINDS, kind
    top = (1 << bit_depth) - 1
    H, W = h + 384, w + 384                              # room for shifts up to +-190 samples, as synth_frame
    rng = np.random.default_rng(seed)

    def texture():
        t = rng.normal(0, 1, (H, W))
        for _ in range(3):
            t = (t + np.roll(t, 1, 0) + np.roll(t, 1, 1) + np.roll(t, -1, 0) + np.roll(t, -1, 1)) / 5
        return (t - t.min()) / (t.max() - t.min())
    yy, xx = np.mgrid[0:H, 0:W]
    fixed = np.zeros((3, H, W), bool)                    # samples the grain must leave at their rail
    if kind == "full_range":
        canvas = np.stack([((texture() - 0.5) * (3.2 if p == 0 else 4.0) + 0.5 + 0.12 * np.sin(xx / (6.0 + p) + yy / 11.0)) * top for p in range(3)])
    else:
        canvas = np.stack([(0.25 + 0.5 * texture()) * top for _ in range(3)])
        r2 = np.random.default_rng(seed + 7)
        for _ in range(H * W // 700):                    # blocks of 0 / top, odd sizes and positions: edges off the 8x8 (and 4x4) grid
            bw, bh = int(r2.integers(3, 29)), int(r2.integers(3, 29))
            bx, by = int(r2.integers(0, W - bw)), int(r2.integers(0, H - bh))
            for p in range(3):
                if p == 0 or r2.random() < 0.6:
                    canvas[p, by:by + bh, bx:bx + bw] = top * int(r2.integers(0, 2))
                    fixed[p, by:by + bh, bx:bx + bw] = True
        for _ in range(H * W // 6000):                   # black fields with single bright samples
            bw, bh = int(r2.integers(12, 40)), int(r2.integers(12, 40))
            bx, by = int(r2.integers(0, W - bw)), int(r2.integers(0, H - bh))
            dots = r2.random((bh, bw)) < 0.04
            for p in range(3):
                canvas[p, by:by + bh, bx:bx + bw] = np.where(dots, top, 0)
                fixed[p, by:by + bh, bx:bx + bw] = True
    oy, ox = 192 + shift[1], 192 + shift[0]
    g = np.random.default_rng((seed * 1000 + shift[0] * 31 + shift[1] + 1) % (1 << 32))
    out = []
    for p in range(3):
        c, f = canvas[p, oy:oy + h, ox:ox + w], fixed[p, oy:oy + h, ox:ox + w]
        if p:
            c, f = c[::2, ::2], f[::2, ::2]
        c = np.where(f, c, c + g.normal(0, 0.004 * top, c.shape))
        out.append(np.clip(np.rint(c), 0, top).astype(np.uint16))
    return O.Frame(*out)


def content_frame(content, h, w, bit_depth=8, seed=0, shift=(0, 0)) -> O.Frame:
    """'synth' (synth_frame) or one of ENVELOPE_KINDS"""
    if content == "synth":
        return synth_frame(h, w, seed, shift=shift, bit_depth=bit_depth)
    return envelope_frame(content, h, w, bit_depth, seed, shift)


def end_fractions(plane, bit_depth):
    """(share of samples at 0, share at 2^bd - 1)"""
    p = np.asarray(plane)
    return float(np.mean(p == 0)), float(np.mean(p == (1 << bit_depth) - 1))


def reaches_both_ends(frame: O.Frame, bit_depth, share=0.0):
    """every plane has more than `share` of its samples at exactly 0 and more than `share` at exactly 2^bd - 1"""
    return all(min(end_fractions(p, bit_depth)) > share for p in (frame.y, frame.u, frame.v))


# stage-parity cases at the ends of the QP range on envelope content, partial CTUs, both bit depths: (w, h, qp, bit depth, me range, kind).
# Every picture of such a case, the I picture included, is coded at the case's QP.
ENVELOPE_QPS = (0, 4, 45, 51)
ENVELOPE_STAGE_CASES = [((136, 72) if (i + i // 4) % 2 == 0 else (72, 104)) + (qp, bd, 8, kind)                    # every QP at both sizes
                        for i, (kind, bd, qp) in enumerate((k, b, q) for k in ENVELOPE_KINDS for b in (8, 10) for q in ENVELOPE_QPS)]


def check_envelope_run(srcs, want, qp, bd):
    """an envelope case must reach what it exists for: both ends of the range in every source plane and in every plane of the reconstruction
    (a share of luma), deblocking that changes samples of the run at the high QPs.  want: run_pipeline's (analysis, deblocked, final, sao) per picture"""
    for i, (src, (a, d, f, _)) in enumerate(zip(srcs, want)):
        assert reaches_both_ends(src, bd, 0.01), f"source {i} misses an end of the range"
        assert min(end_fractions(f.y, bd)) > 0.002 and reaches_both_ends(f, bd), f"reconstruction {i} misses an end of the range"
    if qp >= 45:
        assert any(not d.same(a.rec) for a, d, _, _ in want), "deblocking left every sample alone"


def dtype_for(bit_depth):
    return np.uint8 if bit_depth == 8 else np.uint16


def planes(frame: O.Frame, bit_depth):
    dt = dtype_for(bit_depth)
    return [np.ascontiguousarray(p.astype(dt)) for p in (frame.y, frame.u, frame.v)]


def to_frame(ps) -> O.Frame:
    return O.Frame(*[p.astype(np.uint16) for p in ps])


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def n_ctus(w, h):
    return ((w + 31) // 32) * ((h + 31) // 32)


def psnr(a, b, peak=255.0):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(peak * peak / mse)


def stepped_library():
    """tests/emu/libkernel_emu.so: the kernel sources stepped on the CPU (a test harness: hevc_amd/ never loads it).  Rebuilt when a harness
    source or header, a kernel header, the stage argument builders, the GOP planner, the rate controller or the ABI header is newer than the library"""
    so = EMU_DIR / "libkernel_emu.so"
    sources = sorted(EMU_DIR.glob("*.cpp"))
    deps = sources + list(EMU_DIR.glob("*.h")) + list((ROOT / "hevc_amd" / "csrc" / "kernels").glob("*.h")) + [ROOT / "hevc_amd" / "csrc" / "stage_args.h", ROOT / "hevc_amd" / "csrc" / "gop_plan.h", ROOT / "hevc_amd" / "csrc" / "ratectl.h", ROOT / "include" / "mihevc.h"]
    if not so.exists() or any(d.stat().st_mtime > so.stat().st_mtime for d in deps):
        tmp = so.with_name(f"libkernel_emu.{os.getpid()}.so")                  # renamed into place: a process that has the old one loaded keeps it
        try:
            subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-w", "-pthread", "-o", str(tmp)] + [str(x) for x in sources], check=True)
            os.replace(tmp, so)
        finally:
            tmp.unlink(missing_ok=True)
    return C.CDLL(str(so))


class StageApi:
    """Thin wrapper over the per-stage C-ABI entry points: prefix "mihevc_k_" (the device entries; device: its index) or "emu_" (their stepped twins,
    which take sign_hide after the arguments of every entry that takes cost parameters)."""

    def __init__(self, lib, prefix, device=None, sign_hide=0):
        assert prefix == "emu_" or not sign_hide, "the device entries take sign data hiding from the session configuration only"
        self.lib, self.prefix, self.device, self.sign_hide = lib, prefix, device, sign_hide

    def _call(self, name, *args, cost=True):
        """cost: the entry takes a mihevc_cost_params"""
        f = getattr(self.lib, self.prefix + name)
        tail = [self.sign_hide] if cost and self.prefix == "emu_" else []
        rc = f(*(([self.device] if self.device is not None else []) + list(args) + tail))
        assert rc == 0, f"{self.prefix}{name} -> {rc}"

    def intra(self, src: O.Frame, prm):
        bd = prm.bit_depth
        h, w = src.shape
        s = planes(src, bd)
        o = [np.zeros_like(p) for p in s]
        a = O.Analysis(h, w)
        est = C.c_uint64(0)
        self._call("intra_frame", ptr(s[0]), ptr(s[1]), ptr(s[2]), w, h, C.byref(prm), ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(a.cu), ptr(a.coef_y),
                   ptr(a.coef_u), ptr(a.coef_v), C.byref(est))
        a.rec, a.est = to_frame(o), est.value
        return a

    def intra_plan(self, src: O.Frame, prm):
        """the plan stage alone (mihevc_k_intra_plan / emu_intra_plan): O.INTRA_PLAN_DTYPE per CTU"""
        h, w = src.shape
        s = planes(src, prm.bit_depth)
        plan = np.zeros(n_ctus(w, h), O.INTRA_PLAN_DTYPE)
        self._call("intra_plan", ptr(s[0]), ptr(s[1]), ptr(s[2]), w, h, C.byref(prm), ptr(plan))
        return plan

    def inter(self, src: O.Frame, ref: O.Frame, prm, centers=None):
        return self._inter(src, [ref], prm, [centers])

    def b(self, src: O.Frame, ref0: O.Frame, ref1: O.Frame, prm, centers0=None, centers1=None):
        """B picture between two anchors (mihevc_k_b_frame / emu_b_frame): a.me = (list-0 dump, list-1 dump)"""
        return self._inter(src, [ref0, ref1], prm, [centers0, centers1])

    def _inter(self, src, refs, prm, centers):
        """P (one reference: inter_frame) or B (two: b_frame); centers: one entry per reference, None or per CTU (sx, sy)"""
        bd = prm.bit_depth
        h, w = src.shape
        s, r = planes(src, bd), [p for ref in refs for p in planes(ref, bd)]
        o = [np.zeros_like(p) for p in s]
        a = O.Analysis(h, w)
        me = [np.zeros((n_ctus(w, h), 21, 3), np.int32) for _ in refs]
        est = C.c_uint64(0)
        cen = [np.ascontiguousarray(c, dtype=np.int16) if c is not None else None for c in centers]
        self._call("inter_frame" if len(refs) == 1 else "b_frame", *map(ptr, s), *map(ptr, r), w, h, C.byref(prm), *[ptr(c) if c is not None else None for c in cen],
                   *map(ptr, o), ptr(a.cu), ptr(a.coef_y), ptr(a.coef_u), ptr(a.coef_v), *map(ptr, me), C.byref(est))
        a.rec, a.me, a.est = to_frame(o), me[0] if len(refs) == 1 else tuple(me), est.value
        return a

    def deblock(self, rec: O.Frame, cu, bd):
        r = planes(rec, bd)
        h, w = rec.shape
        self._call("deblock", ptr(r[0]), ptr(r[1]), ptr(r[2]), w, h, ptr(np.ascontiguousarray(cu)), bd, cost=False)
        return to_frame(r)

    def sao(self, src: O.Frame, dbk: O.Frame, prm):
        bd = prm.bit_depth
        h, w = src.shape
        s, d = planes(src, bd), planes(dbk, bd)
        o = [np.zeros_like(p) for p in s]
        sp = np.zeros(n_ctus(w, h), O.SAO_DTYPE)
        self._call("sao", ptr(s[0]), ptr(s[1]), ptr(s[2]), ptr(d[0]), ptr(d[1]), ptr(d[2]), w, h, C.byref(prm), ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(sp))
        return to_frame(o), sp

    def loop_filter(self, src: O.Frame, rec: O.Frame, cu, prm, band=None):
        """deblocking + SAO in one pass over the PRE-deblock reconstruction (the fused CTU program a session runs).  band = (y0, h, halo): emulator only, rows
        [y0, y0 + h) of the picture as one slice whose filters run across the seams (halo bit 0: a slice above, bit 1: below)"""
        bd = prm.bit_depth
        h, w = src.shape
        s, d = planes(src, bd), planes(rec, bd)
        o = [np.zeros_like(p) for p in s]
        cu = np.ascontiguousarray(cu)
        if band is None and self.prefix != "emu_":
            sp = np.zeros(n_ctus(w, h), O.SAO_DTYPE)
            self._call("loop_filter", ptr(s[0]), ptr(s[1]), ptr(s[2]), ptr(d[0]), ptr(d[1]), ptr(d[2]), w, h, ptr(cu), C.byref(prm), ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(sp))
            return to_frame(o), sp
        y0, bh, halo = band if band is not None else (0, h, 0)
        sp = np.zeros(n_ctus(w, bh), O.SAO_DTYPE)
        self._call("loop_filter", ptr(s[0]), ptr(s[1]), ptr(s[2]), ptr(d[0]), ptr(d[1]), ptr(d[2]), w, y0, bh, halo, ptr(cu), C.byref(prm), ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(sp))
        return to_frame(o), sp

    def sao_sse(self, src: O.Frame, dbk: O.Frame, prm):
        """emulator only: SAO with the per-CTU squared-error table the CTU programs leave (SaoArgs::sse_ctu)"""
        bd = prm.bit_depth
        h, w = src.shape
        s, d = planes(src, bd), planes(dbk, bd)
        o = [np.zeros_like(p) for p in s]
        sp = np.zeros(n_ctus(w, h), O.SAO_DTYPE)
        sse = np.full((n_ctus(w, h), 3), 0xffffffff, np.uint32)
        self._call("sao_sse", ptr(s[0]), ptr(s[1]), ptr(s[2]), ptr(d[0]), ptr(d[1]), ptr(d[2]), w, h, C.byref(prm), ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(sp), ptr(sse))
        return to_frame(o), sp, sse


def same_analysis(a, b):
    return (a.rec.same(b.rec) and np.array_equal(a.cu, b.cu) and np.array_equal(a.coef_y, b.coef_y) and
            np.array_equal(a.coef_u, b.coef_u) and np.array_equal(a.coef_v, b.coef_v) and a.est == b.est)


def describe_diff(a, b):
    out = []
    if not np.array_equal(a.cu, b.cu):
        i = np.argwhere(a.cu != b.cu)[0]
        out.append(f"cu[{tuple(i)}]: {a.cu[tuple(i)]} vs {b.cu[tuple(i)]}")
    for n in ("y", "u", "v"):
        pa, pb = getattr(a.rec, n), getattr(b.rec, n)
        if not np.array_equal(pa, pb):
            ys, xs = np.nonzero(pa != pb)
            out.append(f"rec.{n} {len(ys)} diffs, first at x={xs[0]} y={ys[0]}: {pa[ys[0], xs[0]]} vs {pb[ys[0], xs[0]]}")
    for n in ("coef_y", "coef_u", "coef_v"):
        if not np.array_equal(getattr(a, n), getattr(b, n)):
            out.append(f"{n} differs")
    if a.est != b.est:
        out.append(f"rate estimate {a.est} vs {b.est}")
    return "; ".join(out) or "identical"


def run_pipeline(api_or_oracle, srcs, prm_i, prm_p, bd=8):
    """I then P pictures through analysis -> deblock -> SAO with either the oracle module or a StageApi.
    Returns list of (analysis, deblocked, final, sao_params)."""
    out, ref = [], None
    for i, src in enumerate(srcs):
        prm = prm_i if i == 0 else prm_p
        if api_or_oracle is O:
            a = O.analyze_intra(src, prm) if i == 0 else O.analyze_inter(src, ref, prm, dump_me=True)
            d = O.deblock(a.rec, a.cu, bd)
            f, sp = O.sao(src, d, prm)
        else:
            a = api_or_oracle.intra(src, prm) if i == 0 else api_or_oracle.inter(src, ref, prm)
            d = api_or_oracle.deblock(a.rec, a.cu, bd)
            f, sp = api_or_oracle.sao(src, d, prm)
        out.append((a, d, f, sp))
        ref = f
    return out


def idr_positions(n, keyint, lanes=4, balance=True):
    """IDR pictures of a session without scene cuts (hevc_amd/csrc/gop_plan.h gop_plan, one call per chunk; tests/test_gop_plan_cpu.py): chunks of lanes x keyint pictures, every chunk coded as the
    fewest GOPs keyint allows, of near-equal length (cfg.gop_balance, the default) or with an IDR every keyint pictures."""
    out, pos = [], 0
    while pos < n:
        m = min(lanes * keyint, n - pos)
        g = (m + keyint - 1) // keyint
        at = pos
        for j in range(g):
            out.append(at)
            at += (m // g + (j < m % g)) if balance else keyint
        pos += m
    return out


def hrd_arrival_schedule(sizes_bits, keys, bit_rate, init_delays_90k, fps):
    """H.265 C.2.2 (cbr_flag = 0) + C.2.3 for a stream without reordering: picture n is removed at n / fps (the picture timing SEI counts
    clock ticks since the last buffering period), its first bit may enter the CPB no earlier than its removal time minus the initial delay
    announced by the LAST buffering period, and never before the previous picture has fully arrived.  Returns the smallest slack
    (removal time - final arrival time) in seconds: negative = the CPB underflows."""
    t_af, slack, delay = 0.0, 1e9, init_delays_90k[0] / 90000.0
    k = 0
    for n, (bits, key) in enumerate(zip(sizes_bits, keys)):
        if key:
            delay = init_delays_90k[min(k, len(init_delays_90k) - 1)] / 90000.0
            k += 1
        t_r = init_delays_90k[0] / 90000.0 + n / fps
        t_ai = max(t_af, t_r - delay)
        t_af = t_ai + bits / bit_rate
        slack = min(slack, t_r - t_af)
    return slack


# ================================================================ cases of the decision audit (tests/test_analysis_independent.py on the CPU, tests/test_gpu_analysis_independent.py on the device)
def flat_pair(w, h, bd):
    v = 100 << (bd - 8)
    f = O.Frame(np.full((h, w), v), np.full((h // 2, w // 2), v), np.full((h // 2, w // 2), v))
    return f, f.copy()


def periodic_pair(w, h, bd, low_bits=False):
    """period 4 in both directions, the source two samples ahead of the reference: SAD 0 at every d = 2 mod 4, and (-2, -2), (2, -2), (-2, 2), (2, 2) cost the
    same bits.  low_bits (10 bit): every sample of both pictures gets random two low bits, which the search must not see."""
    f, g = np.array([20, 90, 200, 140]), np.array([0, 30, 10, 50])
    yy, xx = np.mgrid[0:h + 2, 0:w + 2]
    big = (f[xx % 4] + g[yy % 4]) << (bd - 8)
    ref, cur = big[:h, :w].copy(), big[2:, 2:].copy()
    if low_bits:
        rng = np.random.default_rng(4)
        ref, cur = (ref & ~3) | rng.integers(0, 4, ref.shape), (cur & ~3) | rng.integers(0, 4, cur.shape)
    c = np.full((h // 2, w // 2), 128 << (bd - 8))
    return O.Frame(cur, c, c), O.Frame(ref, c, c)


SIZES = ((64, 64), (136, 72), (72, 104))
RANGES = (8, 12, 15, 32)
Case = namedtuple("Case", "id w h bd R kind shift centres pre_search")


@functools.lru_cache(maxsize=None)
def _base(w, h, bd):
    return synth_frame(h + 256, w + 256, 5, bit_depth=bd)


def crop(w, h, bd, ox, oy):
    """a window of one larger synthetic picture: crop(s)(x) = crop(0)(x + s), a pure translation"""
    b = _base(w, h, bd)
    return O.Frame(b.y[128 + oy:128 + oy + h, 128 + ox:128 + ox + w].copy(), b.u[64 + oy // 2:64 + (oy + h) // 2, 64 + ox // 2:64 + (ox + w) // 2].copy(),
                   b.v[64 + oy // 2:64 + (oy + h) // 2, 64 + ox // 2:64 + (ox + w) // 2].copy())


def _search_cases():
    """The cross product (kind x R x size x bit depth) is SAMPLED, not run in full: a case's size and bit depth follow from its kind, its R and its index
    within that (kind, R) group alone, so adding or removing a case never moves another one, and every (R, size, bit depth) triple occurs."""
    out, count = [], {}
    kind_no = {"corner": 0, "extra": 1, "past": 2, "flat": 3, "periodic": 4, "lowbits": 5, "centres": 0, "presearch": 3}

    def add(kind, R, shift, centres=None, pre=0):
        i = count.get((kind, R), 0)
        count[(kind, R)] = i + 1
        n = i + kind_no[kind] + RANGES.index(R)
        (w, h), bd = SIZES[n % 3], 10 if kind == "lowbits" else (8, 10)[(n // 3 + i) % 2]
        out.append(Case(f"{kind}-R{R}-{w}x{h}-{bd}bit-{shift[0]}_{shift[1]}", w, h, bd, R, kind, shift, centres, pre))
    for R in RANGES:
        last = -R + A.search_span(R)[0] - 1
        for s in ((-R, -R), (last, -R), (-R, R), (last, R)):
            add("corner", R, s)
        for dx in range(R + 1, last + 1):                                     # the columns the row is widened by: must be found
            add("extra", R, (dx, 1))
        add("past", R, (last + 1, 0))                                         # one position past the last column: must not be found
        for shift in ((0, 0), (0, 0)):                                        # the tie pictures of the pinning tests, twice per R: two (size, bit depth) each
            add("flat", R, shift)
            add("periodic", R, shift)
            add("lowbits", R, shift)
    for R, shifts in ((32, ((-50, 44), (60, -58), (-80, -70), (70, 80), (-50, -60), (40, 52))), (15, ((-50, -60), (44, 50))), (8, ((40, 52),))):
        for s in shifts:
            add("centres", R, s, centres="corners")                           # explicit centres up to +-56: with R = 32 the window leaves the 80-sample border
    for R in RANGES:
        add("presearch", R, (38, -22), pre=1)
        add("presearch", R, (-56, 56), pre=1)
    out.append(Case("corner-R15-136x72-8bit-16_15", 136, 72, 8, 15, "corner", (16, 15), None, 0))      # the one triple the dealing above leaves out
    assert {(c.R, c.w, c.bd) for c in out} == {(R, w, bd) for R in RANGES for w, _ in SIZES for bd in (8, 10)} and len({c.id for c in out}) == len(out)
    return out


SEARCH_CASES = _search_cases()
B_CASE = Case("b-R12-136x72-8bit", 136, 72, 8, 12, "b", ((5, -3), (-6, 4)), None, 0)


def case_pictures(c):
    """(current picture, reference picture)"""
    if c.kind == "flat":
        return flat_pair(c.w, c.h, c.bd)
    if c.kind in ("periodic", "lowbits"):
        return periodic_pair(c.w, c.h, c.bd, low_bits=c.kind == "lowbits")
    return crop(c.w, c.h, c.bd, *c.shift), crop(c.w, c.h, c.bd, 0, 0)


def case_centres(c, salt=0):
    """explicit centres of a case, or None"""
    if c.centres is None:
        return None
    rng = np.random.default_rng(n_ctus(c.w, c.h) + salt)
    pool = np.array([(-56, -56), (56, 56), (-56, 56), (56, -56), (-52, 44), (0, -56), (40, 12)], np.int16)
    cen = pool[rng.integers(0, len(pool), n_ctus(c.w, c.h))]
    cen[0] = (-56, -56)                                                       # CTU 0 at R = 32: reads from -88 on both axes
    cen[-1] = (56, 56)
    return np.ascontiguousarray(cen)


def params_pair(qp, bd, R, **knobs):
    """(oracle parameters, product parameters) for one QP, both from the product's mihevc_cost_params_for_qp"""
    from hevc_amd import _lib
    cp = _lib.cost_params(qp, bd, R)
    prm = O.Params(cp.qp, cp.qp_c, cp.bit_depth, cp.lambda_sad_q4, cp.lambda_q4, cp.me_range)
    for k, v in knobs.items():
        setattr(cp, k, v)
        setattr(prm, k, v)
    return prm, cp


def audit_search(c, cur, ref, lam, centres):
    """the model's dump of one case; with pre_search the centres are the model's own too"""
    if c.pre_search:
        centres = A.pre_search(A.lowres(cur.y, c.bd), A.lowres(ref.y, c.bd))
    return A.integer_search(cur.y, ref.y, c.bd, c.R, lam, centres)


def check_planted(c, me, lam):
    """what the case was built for, on the model's own answer"""
    if c.kind not in ("corner", "extra", "past"):
        return
    hit = (me[:, 5:, 0] == 4 * c.shift[0]) & (me[:, 5:, 1] == 4 * c.shift[1])
    if c.kind == "past":
        assert not (me[:, :, 0] == 4 * c.shift[0]).any(), "a vector outside the candidate set"
    else:
        bits = A.mvd_bits(4 * c.shift[0]) + A.mvd_bits(4 * c.shift[1])
        assert (me[:, 5:, 2][hit] == lam * bits).any(), "the planted displacement is in the candidate set and matches exactly: it must win"


def first_diff(a, b):
    i = np.argwhere((a != b).any(axis=-1))
    return f"{len(i)} nodes differ, first (ctu, node) {i[0].tolist()}: {a[tuple(i[0])].tolist()} vs {b[tuple(i[0])].tolist()}" if len(i) else "equal"


def b_case_pictures():
    c = B_CASE
    return crop(c.w, c.h, c.bd, 5, -3), crop(c.w, c.h, c.bd, 0, 0), crop(c.w, c.h, c.bd, 11, -7)


def b_case_centres():
    return np.tile(np.array([(-4, 2)], np.int16), (n_ctus(B_CASE.w, B_CASE.h), 1))


SAO_QPS = (22, 32, 42)
SaoCase = namedtuple("SaoCase", "id w h bd qp content")
SAO_CASES = [SaoCase(f"{w}x{h}-{bd}bit-qp{qp}", w, h, bd, qp, "synth") for (w, h) in SIZES for bd in (8, 10) for qp in SAO_QPS]
_env = next(e for e in ENVELOPE_STAGE_CASES if e[5] == "rails" and e[3] == 10 and e[2] == 45)
SAO_CASES.append(SaoCase("rails-%dx%d-%dbit-qp%d" % (_env[0], _env[1], _env[3], _env[2]), _env[0], _env[1], _env[3], _env[2], "rails"))
# the encoder's own pictures never made chroma take band offsets or the 45-degree class: a hand-made SAO input that does (planted_sao_input)
SAO_CASES += [SaoCase(f"planted-64x64-{bd}bit-qp27", 64, 64, bd, 27, "planted") for bd in (8, 10)]
CODED_SAO_CASES = [c for c in SAO_CASES if c.content != "planted"]


def sao_case_sources(c):
    """(I picture, P picture): the pictures of the search cases (a translation by (3, 1)), or envelope content with samples at both rails"""
    if c.content == "synth":
        return crop(c.w, c.h, c.bd, 0, 0), crop(c.w, c.h, c.bd, 3, 1)
    return tuple(envelope_frame(c.content, c.h, c.w, c.bd, 3, shift=(2 * i, i)) for i in range(2))


def planted_sao_input(c):
    """(source, "deblocked"): luma untouched.  Chroma CTB 0: Cb 3 and Cr 2 grey levels too low everywhere: band offsets.  Chroma CTB 1: the source is a ramp
    along x + y, the deblocked picture adds +-2 of noise: the two neighbours of the 45-degree class share the ramp's value, so that class alone sees the noise as
    minima and maxima; to every other class the ramp makes each sample a monotone step (category 0)."""
    sc = 1 << (c.bd - 8)
    src = crop(c.w, c.h, c.bd, 0, 0)
    yy, xx = np.mgrid[0:16, 0:16]
    ramp = (8 * (xx + yy)) * sc
    src.u[0:16, 16:32], src.v[0:16, 16:32] = ramp, ramp[::-1, ::-1]
    d = src.copy()
    d.u[0:16, 0:16] -= 3 * sc
    d.v[0:16, 0:16] -= 2 * sc
    rng = np.random.default_rng(8)
    d.u[0:16, 16:32] += (2 * sc * rng.integers(0, 3, (16, 16))).astype(np.uint16)
    d.v[0:16, 16:32] += (2 * sc * rng.integers(0, 3, (16, 16))).astype(np.uint16)
    return src, d


def planes3(f):
    return f.y, f.u, f.v


def sao_kinds(sp):
    """what a parameter array exercises: 'off', 'band', 'edge0'..'edge3', per luma / chroma"""
    out = set()
    for i in range(2):
        for t, k in zip(sp["type"][:, i], sp["eo_class"][:, i]):
            out.add(("luma ", "chroma ")[i] + ("off", "band", "edge%d" % k)[t])
    return out


ALL_SAO_KINDS = {p + k for p in ("luma ", "chroma ") for k in ("off", "band", "edge0", "edge1", "edge2", "edge3")}


def sao_diff(a, b):
    i = np.nonzero([x.tobytes() != y.tobytes() for x, y in zip(a, b)])[0]
    return f"{len(i)} CTUs differ, first {i[0]}: {a[i[0]]} vs {b[i[0]]}" if len(i) else "equal"


# ================================================================ cases of the intra plan audit (tests/test_intra_plan_independent.py on the CPU, tests/test_gpu_intra_plan_independent.py on the device)
PLAN_QPS = (22, 32, 42)
PlanCase = namedtuple("PlanCase", "id w h bd qp chroma_modes content tiles lam", defaults=(None,))      # lam: None, or (lambda_sad_q4, lambda_q4) in place of the QP's own


def _plan_cases():
    out = [PlanCase(f"{w}x{h}-{bd}bit-qp{qp}-cm{cm}", w, h, bd, qp, cm, "synth", (1, 1)) for (w, h) in SIZES for bd in (8, 10) for qp in PLAN_QPS for cm in (0, 1)]
    for e in ENVELOPE_STAGE_CASES:                                            # rails content at QP 45, both bit depths
        if e[5] == "rails" and e[2] == 45:
            out.append(PlanCase("rails-%dx%d-%dbit-qp45" % (e[0], e[1], e[3]), e[0], e[1], e[3], 45, 1, "rails", (1, 1)))
    out += [PlanCase(f"drawn{i}-224x160-8bit-qp27", 224, 160, 8, 27, 1, f"drawn{i}", (1, 1)) for i in range(2)]     # the hand-drawn all-modes pictures
    out.append(PlanCase("fan-224x160-10bit-qp30", 224, 160, 10, 30, 1, "fan", (1, 1)))
    out.append(PlanCase("tiles2x2-40x40-8bit-qp32", 40, 40, 8, 32, 1, "synth", (2, 2)))     # 2 x 2 CTUs: the smallest picture a 2 x 2 grid fits
    out.append(PlanCase("tiles2x2-136x72-10bit-qp27", 136, 72, 10, 27, 1, "synth", (2, 2)))
    # the hand-made pictures of tests/test_intra_plan_independent.py whose answer hangs on an exact tie or on a threshold, so that the device meets them too:
    # lambda_q4 = 0 on a flat CTU and on column stripes (whole == split == 0 at both levels of the tree), the DM tie (lambda_sad_q4 8: DM and horizontal cost
    # 3000 each in CTU 3, node 8) and one less, the 32x32 reference line that passes the strong-smoothing test by one and the one that misses it
    out.append(PlanCase("flat-32x32-8bit-lam0", 32, 32, 8, 22, 1, "flat", (1, 1), (38, 0)))
    out.append(PlanCase("stripes-64x64-8bit-lam0", 64, 64, 8, 22, 1, "stripes", (1, 1), (38, 0)))
    out.append(PlanCase("dmtie-64x64-8bit-lamsad8", 64, 64, 8, 22, 1, "synth", (1, 1), (8, 92)))
    out.append(PlanCase("dmtie-64x64-8bit-lamsad7", 64, 64, 8, 22, 1, "synth", (1, 1), (7, 92)))
    for bd in (8, 10):
        out += [PlanCase(f"line{d}-96x64-{bd}bit-qp22", 96, 64, bd, 22, 1, f"line{d}", (1, 1)) for d in ((7, 8) if bd == 8 else (31, 32))]
    assert len({c.id for c in out}) == len(out)
    return out


PLAN_CASES = _plan_cases()
# the device file's share: 64x64 and 136x72, both bit depths, QP 22 and 42, chroma modes on, and the tiled cases
GPU_PLAN_CASES = [c for c in PLAN_CASES if (c.content == "synth" and c.tiles == (1, 1) and (c.w, c.h) in ((64, 64), (136, 72)) and c.qp in (22, 42) and c.chroma_modes) or
                  c.tiles != (1, 1) or c.lam is not None or c.content.startswith("line")]


def fan_picture(w, h, bd):
    """every CTU striped along the direction of one angular mode, 2..34 in raster order (then planar-like and flat CTUs): along a vertical mode of angle A
    (Table 8-4, in 1/32 sample per row) the picture is constant on the lines x + y A / 32 = const, along a horizontal mode on y + x A / 32 = const.  The
    encoder's own pictures and the drawn ones leave some of the 35 modes unpicked; here a block inside CTU k has mode 2 + k as its exact predictor."""
    angle = (32, 26, 21, 17, 13, 9, 5, 2, 0, -2, -5, -9, -13, -17, -21, -26, -32, -26, -21, -17, -13, -9, -5, -2, 0, 2, 5, 9, 13, 17, 21, 26, 32)
    rng = np.random.default_rng(12)
    top = (1 << bd) - 1
    prof = np.clip(np.repeat(rng.integers(top // 8, top - top // 8, 64), 3)[:160] + rng.integers(-2, 3, 160), 0, top)      # steps three lines wide
    yy, xx = np.mgrid[0:32, 0:32]
    y = np.zeros((h, w), np.int64)
    for k, (cy, cx) in enumerate((cy, cx) for cy in range(0, h, 32) for cx in range(0, w, 32)):
        if k < 33:
            a = angle[k]
            t = (32 * xx + a * yy if k + 2 >= 18 else 32 * yy + a * xx) + 32 * 32
            f = t % 32
            blk = ((32 - f) * prof[t // 32] + f * prof[t // 32 + 1] + 16) >> 5
        else:
            blk = np.full((32, 32), prof[k]) + (xx + yy if k == 33 else 0)
        y[cy:cy + 32, cx:cx + 32] = blk[:h - cy, :w - cx]
    c = (y[::2, ::2] + y[1::2, 1::2]) // 2
    return O.Frame(y, c, top - c)


STRIPE = (40, 200, 90, 160, 20, 230, 120, 60)
PLAN_SOURCES = {}            # content -> function(w, h, bd) -> O.Frame, for pictures a test module makes (the drawn pictures: tests/test_intra_plan_independent.py)


def smoothing_line_picture(w, h, bd, d):
    """flat but for two samples of the row above CTU (1, 1): the 32x32 node's top reference line has |corner + last - 2 middle| = d (8.4.4.2.3)"""
    v = 100 << (bd - 8)
    y = np.full((h, w), v)
    y[31, 63], y[31, 95] = v - 3, v + d - 6
    c = np.full((h // 2, w // 2), 1 << (bd - 1))
    return O.Frame(y, c, c)


@functools.lru_cache(maxsize=None)
def plan_case_source(content, w, h, bd):
    if content in PLAN_SOURCES:
        return PLAN_SOURCES[content](w, h, bd)
    if content == "synth":
        return crop(w, h, bd, 0, 0)
    if content == "fan":
        return fan_picture(w, h, bd)
    if content == "flat":
        v = np.full((h, w), 1 << (bd - 1))
        return O.Frame(v, v[::2, ::2], v[::2, ::2])
    if content == "stripes":
        col = np.tile(np.array(STRIPE * (w // 8)) << (bd - 8), (h, 1))
        return O.Frame(col, col[::2, ::2], col[::2, ::2])
    if content.startswith("line"):
        return smoothing_line_picture(w, h, bd, int(content[4:]))
    return envelope_frame(content, h, w, bd, 3)


PLAN_COVERAGE = collections.Counter()                            # what the MODEL reached over every case it was asked for


@functools.lru_cache(maxsize=None)
def plan_model(content, w, h, bd, tiles):
    """the model of one picture: the part of its work that does not depend on the cost parameters is done once for all QPs"""
    from tests import hevc_intra_plan as M
    return M.IntraPlanModel(planes3(plan_case_source(content, w, h, bd)), bd, tiles[0], tiles[1], PLAN_COVERAGE)


@functools.lru_cache(maxsize=None)
def plan_case_want(c):
    """(model's plan, oracle parameters, product parameters)"""
    knobs = dict(chroma_modes=c.chroma_modes, tile_cols=c.tiles[0], tile_rows=c.tiles[1])
    if c.lam is not None:
        knobs.update(lambda_sad_q4=c.lam[0], lambda_q4=c.lam[1])
    prm, cp = params_pair(c.qp, c.bd, 8, **knobs)
    return plan_model(c.content, c.w, c.h, c.bd, c.tiles).plan(cp.qp, cp.qp_c, cp.lambda_sad_q4, cp.lambda_q4, c.chroma_modes), prm, cp


def plan_diff(a, b):
    for ctu in range(len(a)):
        for f in ("chosen", "mode", "cmode", "pad"):
            if not np.array_equal(a[ctu][f], b[ctu][f]):
                nd = np.nonzero(np.atleast_1d(a[ctu][f] != b[ctu][f]))[0]
                return f"CTU {ctu} {f}: nodes {nd.tolist()}: {np.atleast_1d(a[ctu][f])[nd].tolist()} vs {np.atleast_1d(b[ctu][f])[nd].tolist()}"
    return "equal"


def check_records_carry_the_plan(plan, cu, w, h, nxn):
    """every CU record lies in a chosen leaf of its CTU's plan and has that leaf's size; its modes are the leaf's (records of an NxN CU: the size only)"""
    from tests import hevc_analysis as A2
    wc = (w + 31) // 32
    seen = np.zeros(cu.shape, bool)
    for ctu in range(len(plan)):
        x0, y0 = ctu % wc * 32, ctu // wc * 32
        for nd, (x, y, n) in enumerate(A2.NODES):
            if not plan[ctu]["chosen"][nd]:
                continue
            r = cu[(y0 + y) // 8:(y0 + y + n) // 8, (x0 + x) // 8:(x0 + x + n) // 8]
            assert r.size == (n // 8) ** 2 and not seen[(y0 + y) // 8:(y0 + y + n) // 8, (x0 + x) // 8:(x0 + x + n) // 8].any(), (ctu, nd)
            seen[(y0 + y) // 8:(y0 + y + n) // 8, (x0 + x) // 8:(x0 + x + n) // 8] = True
            assert (r["log2_size"] == n.bit_length() - 1).all(), f"CTU {ctu} node {nd}: the plan's leaf is {n}, the records say {r['log2_size'].tolist()}"
            assert not (r["flags"] & 1).any()
            is_nxn = (r["flags"] & 16) != 0
            assert nxn or not is_nxn.any()
            keep = ~is_nxn
            assert (r["intra_mode"][..., 0][keep] == plan[ctu]["mode"][nd]).all() and (r["chroma_mode"][keep] == plan[ctu]["cmode"][nd]).all(), \
                f"CTU {ctu} node {nd}: planned {plan[ctu]['mode'][nd]} / {plan[ctu]['cmode'][nd]}, coded {r['intra_mode'][..., 0].tolist()} / {r['chroma_mode'].tolist()}"
    assert seen.all(), "a CU record outside every chosen leaf"


# ================================================================ cases of the intra code audit: the code stage, the NxN trial and the intra second pass of P pictures
# (tests/test_intra_code_independent.py on the CPU, tests/test_gpu_intra_code_independent.py on the device; the model is tests/hevc_intra_code.py)
# An I case is a case of the plan audit (its picture, QP, bit depth, chroma_modes, tile grid and lambdas; the model's own plan is what the model codes) + intra_nxn.
CodeCase = namedtuple("CodeCase", "id plan nxn sign_hide", defaults=(0,))
# A P case: content "patched" = a translation by (3, 1) of the reference with four pasted 64x32 patches, two of unrelated content and two of the reference's own content
# from 60 samples away (where they fit the picture: they are cut at its edges), in CTU rows 0 and 2 and CTU columns 0-1 and 3-4, so that isolated candidates and pairs
# fill both rounds; "noise" = two patches of white noise, which intra prediction codes no better than the search does; "occluded" = tests/test_bitstream_cpu.py's clip,
# one connected patch, most of whose CTUs are never tried; "unrelated" = a picture against a black reference: every CTU is a candidate.
PCodeCase = namedtuple("PCodeCase", "id w h bd qp nxn rdo_zero content seed tiles mc sign_hide", defaults=((1, 1), (0, 0), 0))


def _code_cases():
    out = []
    for c in PLAN_CASES:
        if c.lam is not None or c.content.startswith(("line", "drawn")):
            continue
        if c.content == "synth" and c.tiles == (1, 1):                         # the matrix: 3 sizes x 2 bit depths x 3 QPs x chroma_modes 0 / 1, x intra_nxn 0 / 1
            out += [CodeCase(f"{c.id}-nxn{nxn}", c, nxn) for nxn in (0, 1)]
        else:                                                                  # rails at QP 45 (both depths), the two tile grids, the fan picture
            out += [CodeCase(f"{c.id}-nxn{nxn}", c, nxn) for nxn in ((0, 1) if c.content == "rails" or c.w == 136 else (1,))]
    # low QP and lambda_q4 = 0: J is 16 SSE alone and most CUs rebuild their source exactly both ways, so J_nxn == J_2Nx2N occurs and the 2Nx2N coding must stay
    out.append(CodeCase("jtie-64x64-8bit-qp4-lam0-nxn1", PlanCase("64x64-8bit-qp4-lam0", 64, 64, 8, 4, 1, "synth", (1, 1), (10, 0)), 1))
    out.append(CodeCase("jtie-72x104-10bit-qp4-lam0-nxn1", PlanCase("72x104-10bit-qp4-lam0", 72, 104, 10, 4, 1, "synth", (1, 1), (40, 0)), 1))
    assert len({c.id for c in out}) == len(out)
    return out


CODE_CASES = _code_cases()
# sign data hiding: the oracle has none and the device entries take none, so these run against the stepped kernels only
CODE_SIGN_HIDE_CASES = [CodeCase("sdh-136x72-8bit-qp22-cm1-nxn1", next(c for c in PLAN_CASES if c.id == "136x72-8bit-qp22-cm1"), 1, 1),
                        CodeCase("sdh-72x104-10bit-qp32-cm1-nxn1", next(c for c in PLAN_CASES if c.id == "72x104-10bit-qp32-cm1"), 1, 1)]
# the device file's share: 64x64 and 136x72, both bit depths, QP 22 / 42, chroma modes and NxN on; the tiled cases; the J ties
GPU_CODE_CASES = [c for c in CODE_CASES if c.nxn and ((c.plan.content == "synth" and c.plan.tiles == (1, 1) and c.plan.lam is None and (c.plan.w, c.plan.h) in ((64, 64), (136, 72)) and
                                                       c.plan.qp in (22, 42) and c.plan.chroma_modes) or c.plan.tiles != (1, 1) or c.plan.lam is not None)]


def _p_code_cases():
    out, i = [], 0
    for (w, h) in ((136, 72), (72, 104)):
        for bd in (8, 10):
            for nxn in (0, 1):
                for rz in (0, 1):
                    content = ("patched", "occluded", "patched", "noise")[i % 4] if (i // 4) % 2 == 0 else ("occluded", "patched", "noise", "patched")[i % 4]
                    qp = (27, 24, 32, 37)[(i + i // 4) % 4]
                    out.append(PCodeCase(f"{content}-{w}x{h}-{bd}bit-qp{qp}-nxn{nxn}-rz{rz}", w, h, bd, qp, nxn, rz, content, 1 + i))
                    i += 1
    out.append(PCodeCase("patched-136x104-8bit-qp24-nxn1-rz1-tiles2x2", 136, 104, 8, 24, 1, 1, "patched", 30, (2, 2)))
    out.append(PCodeCase("patched-136x72-10bit-qp27-nxn1-rz1-slice11", 136, 72, 10, 27, 1, 1, "patched", 31, (1, 1), (1, 1)))
    out.append(PCodeCase("unrelated-136x72-8bit-qp27-nxn1-rz1", 136, 72, 8, 27, 1, 1, "unrelated", 32))
    assert len({c.id for c in out}) == len(out)
    return out


P_CODE_CASES = _p_code_cases()
P_CODE_SIGN_HIDE_CASES = [PCodeCase("sdh-patched-136x72-8bit-qp24-nxn1-rz1", 136, 72, 8, 24, 1, 1, "patched", 40, sign_hide=1),
                          PCodeCase("sdh-patched-72x104-10bit-qp27-nxn1-rz0", 72, 104, 10, 27, 1, 0, "patched", 41, sign_hide=1)]
GPU_P_CODE_CASES = [c for c in P_CODE_CASES if c.id in ("patched-136x72-8bit-qp27-nxn0-rz0", "patched-136x72-10bit-qp27-nxn1-rz1", "patched-136x104-8bit-qp24-nxn1-rz1-tiles2x2",
                                                        "noise-136x72-8bit-qp37-nxn1-rz1")]
assert len(GPU_P_CODE_CASES) == 4


@functools.lru_cache(maxsize=None)
def p_code_case_pictures(c):
    """(current picture, reference picture)"""
    if c.content == "occluded":
        from tests.test_bitstream_cpu import occluded_clip
        srcs = occluded_clip(c.w, c.h, c.bd)
        return srcs[1 + c.seed % 2], srcs[0]
    ref = crop(c.w, c.h, c.bd, 0, 0)
    if c.content == "unrelated":                                 # against a black reference the inter cost holds the DC term that the activity leaves out: every CTU is a candidate
        return synth_frame(c.h, c.w, seed=900 + c.seed, bit_depth=c.bd), O.Frame(*[np.zeros_like(p) for p in planes3(ref)])
    cur = crop(c.w, c.h, c.bd, 3, 1)
    other, far = synth_frame(c.h, c.w, seed=900 + c.seed, bit_depth=c.bd), crop(c.w, c.h, c.bd, 60, -45)
    rng = np.random.default_rng(c.seed)
    noise = O.Frame(*[rng.integers(0, 1 << c.bd, p.shape) for p in planes3(cur)])
    boxes = ((0, 0, noise), (96, 0, noise)) if c.content == "noise" else ((0, 0, other), (96, 0, far), (0, 64, far), (96, 64, other))
    for x, y, s in boxes:
        for p, q, sh in ((cur.y, s.y, 0), (cur.u, s.u, 1), (cur.v, s.v, 1)):
            p[y >> sh:(y + 32) >> sh, x >> sh:(x + 64) >> sh] = q[y >> sh:(y + 32) >> sh, x >> sh:(x + 64) >> sh]
    return cur, ref


def model_params(cp, sign_hide=0):
    """the cost parameters as the model takes them: the product's fields + sign_hide (which the stepped entries take as an argument of its own)"""
    import types
    return types.SimpleNamespace(sign_hide=sign_hide, **{f: int(getattr(cp, f)) for f, _ in cp._fields_})


CODE_COVERAGE = collections.Counter()                            # what the MODEL reached over CODE_CASES and P_CODE_CASES, each counted once (the wants are kept)


def code_case_params(c):
    """(oracle parameters, product parameters) of an I case"""
    _, prm0, cp0 = plan_case_want(c.plan)
    prm, cp = type(prm0).from_buffer_copy(prm0), type(cp0).from_buffer_copy(cp0)
    prm.intra_nxn = cp.intra_nxn = c.nxn
    return prm, cp


@functools.lru_cache(maxsize=None)
def code_case_want(c, list_from_plan=False):
    """the model's Result of an I case: computed once.  list_from_plan: the binding test's switch (not counted in CODE_COVERAGE)"""
    from tests import hevc_intra_code as M
    plan = plan_case_want(c.plan)[0]
    _, cp = code_case_params(c)
    src = plan_case_source(c.plan.content, c.plan.w, c.plan.h, c.plan.bd)
    counted = c in CODE_CASES and not list_from_plan                 # the sign-hiding cases, their plain twins and the binding test's runs are not counted
    return M.code_picture(planes3(src), plan, model_params(cp, c.sign_hide), cov=CODE_COVERAGE if counted else None, list_from_plan=list_from_plan)


def p_code_case_params(c):
    return params_pair(c.qp, c.bd, 8, intra_in_p=1, intra_nxn=c.nxn, chroma_modes=1, rdo_zero=c.rdo_zero, tile_cols=c.tiles[0], tile_rows=c.tiles[1], mc_top=c.mc[0], mc_bottom=c.mc[1])


@functools.lru_cache(maxsize=None)
def p_code_case_want(c, list_from_plan=False, activity_with_dc=False):
    from tests import hevc_intra_code as M
    _, cp = p_code_case_params(c)
    cur, ref = p_code_case_pictures(c)
    counted = c in P_CODE_CASES and not list_from_plan and not activity_with_dc
    return M.second_pass(planes3(cur), planes3(ref), model_params(cp, c.sign_hide), cov=CODE_COVERAGE if counted else None,
                         list_from_plan=list_from_plan, activity_with_dc=activity_with_dc)


# ================================================================ cases of the inter CTU program's audit (tests/test_inter_cu_independent.py on the CPU, tests/test_gpu_inter_cu_independent.py on the device)
# content: "crop" = the search audit's pure translation by `shift`; "flat"; "warpG" = every G x G block of the current picture is the reference predicted at a
# quarter-sample vector of its own through the standard's filter (tests/hevc_recon.py), + noise of +-`noise`; B pictures ("b-..."): the blocks are predicted from
# list 0, list 1 or both.  "soft-" in front: the reference(s) at an eighth of their contrast, so that the ring's candidates predict nearly the same block and the
# noise decides between them by a few units of SATD.  mvs: None = drawn per block from `seed` (|mv| < 4 me_range), or the vectors themselves, dealt to the blocks in raster order.
# lam: None = the lambdas of the QP, or (lambda_sad_q4, lambda_q4) with None for the QP's own.  plant: ((plane, x, y, n, dc, e), ...): after everything else the n x n block at
# (x, y) of the current picture's plane gets dc added to every sample and (n = 8) e x (+ - - + + - - +) by rows: the fifth basis function of the 8-point transform down
# the columns, so that an exactly predicted block has the coefficients (0, 0) and (4, 0) alone
InterCase = namedtuple("InterCase", "id w h bd R qp content seed shift noise mvs centres pre_search rdo_zero mc lam rdo_cg plant")
PLANT_ROWS = (1, -1, -1, 1, 1, -1, -1, 1)


def inter_case(id, w, h, bd, R, qp, content, seed=1, shift=(0, 0), noise=0, mvs=None, centres=None, pre_search=0, rdo_zero=0, mc=(0, 0), lam=None, rdo_cg=0, plant=()):
    return InterCase(id, w, h, bd, R, qp, content, seed, shift, noise, mvs, centres, pre_search, rdo_zero, mc, lam, rdo_cg, plant)


def warp_picture(refs, w, h, bd, g, seed, noise, mvs, lists, reach):
    """refs: one or two O.Frame; every g x g block of the result is 8.5.3.3.3 + 8.5.3.3.4.2 of the references (reads clamped to the picture, as a decoder's)
    at the block's own vector(s); lists: per block 0 / 1 / 2 (list 0, list 1, both), dealt in raster order like mvs.  -> (picture, [(x, y, lists, mv0, mv1)])"""
    from tests import hevc_recon as HR
    rng = np.random.default_rng(seed)
    out = [np.zeros((h, w), np.int64), np.zeros((h // 2, w // 2), np.int64), np.zeros((h // 2, w // 2), np.int64)]
    rp = [planes3(r) for r in refs]
    blocks = []
    for i, (y, x) in enumerate((y, x) for y in range(0, h, g) for x in range(0, w, g)):
        mv = [tuple(mvs[(2 * i + l) % len(mvs)]) if mvs is not None else tuple(int(v) for v in rng.integers(-reach, reach + 1, 2)) for l in range(2)]
        mode = lists[i % len(lists)]
        bw, bh = min(g, w - x), min(g, h - y)
        n = max(bw, bh)                                                  # (a block cut by the picture's edge is predicted whole and cropped)
        for c in range(3):
            sh = 1 if c else 0
            mc = HR.mc_chroma if c else HR.mc_luma
            p = HR.weighted_default([mc(rp[l][c].astype(np.int64), x >> sh, y >> sh, n >> sh, mv[l], bd) for l in range(2) if mode == 2 or mode == l], bd)
            out[c][y >> sh:(y + bh) >> sh, x >> sh:(x + bw) >> sh] = p[:bh >> sh, :bw >> sh]
        blocks.append((x, y, mode, mv[0], mv[1]))
    if noise:
        out = [np.clip(p + rng.integers(-noise, noise + 1, p.shape), 0, (1 << bd) - 1) for p in out]
    return O.Frame(*out), blocks


def inter_case_pictures(c):
    """(current picture, (reference,) or (list-0 anchor, list-1 anchor), planted blocks or None)"""
    cur, refs, blocks = _inter_case_pictures(c._replace(id="", qp=0, lam=None, rdo_zero=0, rdo_cg=0))       # (what the pictures do not depend on)
    return cur, refs, blocks


@functools.lru_cache(maxsize=None)
def _inter_case_pictures(c):
    cur, refs, blocks = _inter_case_pictures_unplanted(c._replace(plant=()))
    if c.plant:
        planes = [p.astype(np.int64) for p in planes3(cur)]
        for plane, x, y, n, dc, e in c.plant:
            assert n == 8 or not e
            planes[plane][y:y + n, x:x + n] += dc + e * np.array(PLANT_ROWS * (n // 8))[:, None]
            assert planes[plane].min() >= 0 and planes[plane].max() < 1 << c.bd
        cur = O.Frame(*planes)
    return cur, refs, blocks


@functools.lru_cache(maxsize=None)
def _inter_case_pictures_unplanted(c):
    if c.content == "flat":
        cur, ref = flat_pair(c.w, c.h, c.bd)
        return cur, (ref,), None
    if c.content == "crop":
        return crop(c.w, c.h, c.bd, *c.shift), (crop(c.w, c.h, c.bd, 0, 0),), None
    kind, g = c.content.rstrip("0123456789"), int(c.content[len(c.content.rstrip("0123456789")):])
    soft = kind.startswith("soft-")
    kind = kind[5:] if soft else kind

    def anchor(ox, oy):
        f = crop(c.w, c.h, c.bd, ox, oy)
        if soft:
            mid = 128 << (c.bd - 8)
            f = O.Frame(*[(p.astype(np.int64) - mid) // 8 + mid for p in (f.y, f.u, f.v)])
        return f
    ref0 = anchor(0, 0)
    reach = 4 * c.R - 6
    if kind == "warp":
        cur, blocks = warp_picture([ref0], c.w, c.h, c.bd, g, c.seed, c.noise, c.mvs, (0,), reach)
        return cur, (ref0,), blocks
    if kind in ("b-avg", "b-first", "b-second"):                  # the pins: the second anchor is the first, 2 samples to the right and 1 up, + noise of +-4, so both lists find
        rng = np.random.default_rng(8)                             # the planted vectors (list 1's = list 0's - (8, -4)), each with an error that their average does not have
        ref1 = O.Frame(*[np.clip(p.astype(np.int64) + rng.integers(-4, 5, p.shape) * (1 << (c.bd - 8)), 0, (1 << c.bd) - 1) for p in planes3(crop(c.w, c.h, c.bd, 2, -1))])
    else:
        ref1 = ref0 if kind == "b-same" else anchor(9, -5)
    lists = {"b-avg": (2,), "b-first": (0,), "b-second": (1,), "b-same": (0,), "b-mix": (2, 0, 1, 1, 2, 0, 0)}[kind]
    cur, blocks = warp_picture([ref0, ref1], c.w, c.h, c.bd, g, c.seed, c.noise, c.mvs, lists, reach)
    return cur, (ref0, ref1), blocks


def inter_case_centres(c, n_refs):
    """per reference None or (n_ctu, 2)"""
    if c.centres is None:
        return [None] * n_refs
    if c.centres == "corners":
        return [case_centres(c, salt=l) for l in range(n_refs)]
    return [np.tile(np.array([c.centres[l]], np.int16), (n_ctus(c.w, c.h), 1)) for l in range(n_refs)]


def inter_case_params(c):
    knobs = dict(pre_search=c.pre_search, rdo_zero=c.rdo_zero, mc_top=c.mc[0], mc_bottom=c.mc[1], rdo_cg=c.rdo_cg)
    if c.lam is not None:
        knobs.update({k: v for k, v in (("lambda_sad_q4", c.lam[0]), ("lambda_q4", c.lam[1])) if v is not None})
    return params_pair(c.qp, c.bd, c.R, **knobs)


INTER_COVERAGE = {}                                              # case id -> what the MODEL reached in it


@functools.lru_cache(maxsize=None)
def inter_case_want(c, sign_hide=0):
    """(the model's analysis, the integer tables it started from, the centres given to the entry points): computed once per case.  sign_hide = 1 (no field of a case:
    the frame stage entries and the oracle do not take it; the stepped kernels do): counted under INTER_COVERAGE[c.id + "+sdh"]"""
    from tests import hevc_inter_cu as M
    _, cp = inter_case_params(c)
    cur, refs, _ = inter_case_pictures(c)
    cen = inter_case_centres(c, len(refs))
    given = list(cen)
    if c.pre_search:
        cen = [A.pre_search(A.lowres(cur.y, c.bd), A.lowres(refs[0].y, c.bd))]
    cen_search = cen
    if c.mc[0] or c.mc[1]:                                       # a slice: the search runs around the clamped centre
        wc = (c.w + 31) // 32
        cen_search = []
        for k in cen:
            k = np.zeros((n_ctus(c.w, c.h), 2), np.int16) if k is None else np.array(k, np.int16)
            for i in range(len(k)):
                k[i, 1] = M.clamp_centre_y(int(k[i, 1]), i // wc * 32, c.R, c.h, *c.mc)
            cen_search.append(k)
    me = [M.integer_table(cur.y, r.y, c.bd, c.R, cp.lambda_sad_q4, k, *c.mc) for r, k in zip(refs, cen_search)]
    cov = INTER_COVERAGE[c.id + ("+sdh" if sign_hide else "")] = collections.Counter()
    want = M.analyse(planes3(cur), [planes3(r) for r in refs], me, c.bd, cp.qp, cp.qp_c, cp.lambda_sad_q4, cp.lambda_q4, c.R, cen, c.rdo_zero, c.mc[0], c.mc[1], cov, rdo_cg=c.rdo_cg,
                     sign_hide=sign_hide)
    return want, me, given


def _inter_cases():
    out = []
    # the matrix: size x bit depth x me_range x QP x rdo_zero; content and noise follow from the index so that every grid size meets every size and depth
    i = 0
    for (w, h) in SIZES:
        for bd in (8, 10):
            for R in (8, 15):
                for qp in SAO_QPS:
                    for rz in (0, 1):
                        g = (8, 16, 32)[(i // 2 + i // 12) % 3]
                        out.append(inter_case(f"warp{g}-{w}x{h}-{bd}bit-R{R}-qp{qp}-rz{rz}", w, h, bd, R, qp, f"warp{g}", seed=i // 2, noise=(1 + i // 2 % 3) << (bd - 8), rdo_zero=rz))
                        i += 1
    for k, (w, h) in enumerate(SIZES):                               # translations, explicit centres up to +-56, the pre-search
        bd = (8, 10)[k % 2]
        out.append(inter_case(f"crop-{w}x{h}-{bd}bit-R8", w, h, bd, 8, 27, "crop", shift=(5, -3), rdo_zero=1))
        out.append(inter_case(f"centres-{w}x{h}-{bd}bit-R15", w, h, bd, 15, 32, "crop", shift=(-50, 44), centres="corners", rdo_zero=k & 1))
        out.append(inter_case(f"centres-{w}x{h}-{18 - bd}bit-R8", w, h, 18 - bd, 8, 22, "crop", shift=(40, 52), centres="corners", rdo_zero=1 - (k & 1)))
        out.append(inter_case(f"presearch-{w}x{h}-{bd}bit-R8", w, h, bd, 8, 32, "crop", shift=(38, -22), pre_search=1, rdo_zero=1))
        out.append(inter_case(f"presearch-{w}x{h}-{18 - bd}bit-R15", w, h, 18 - bd, 15, 27, "crop", shift=(-56, 56), pre_search=1))
    for k, mc in enumerate(((1, 0), (0, 1), (1, 1))):                # slices: vertical motion planted in every block, towards and past the slice's rows
        for j, (w, h) in enumerate(SIZES):
            bd = (8, 10)[(k + j) % 2]
            out.append(inter_case(f"slice{mc[0]}{mc[1]}-{w}x{h}-{bd}bit", w, h, bd, 8, 27, "warp8" if j == 1 else "warp16", seed=40 + 3 * k + j, noise=1 << (bd - 8),
                                  rdo_zero=j & 1, mc=mc, centres=None if j else ((3, -5),), pre_search=1 if j == 2 else 0))
    for k, (w, h) in enumerate(SIZES):                               # ties: lambda_sad_q4 = 0
        bd = (8, 10)[k % 2]
        out.append(inter_case(f"lam0-flat-{w}x{h}-{bd}bit", w, h, bd, 8, 27, "flat", lam=(0, 60)))
        out.append(inter_case(f"lam0-warp16-{w}x{h}-{bd}bit", w, h, bd, 8, 27, "warp16", seed=70 + k, lam=(0, 60), rdo_zero=1))
        out.append(inter_case(f"lam0-warp8-{w}x{h}-{18 - bd}bit", w, h, 18 - bd, 15, 32, "warp8", seed=80 + k, noise=1 << (10 - bd), lam=(0, 200 << (2 * (10 - bd))), rdo_zero=1))
    out.append(inter_case("flat-64x64-8bit", 64, 64, 8, 8, 27, "flat"))
    # B pictures
    for k, (w, h) in enumerate(SIZES):
        for j, bd in enumerate((8, 10)):
            kind = ("b-mix", "b-same", "b-mix")[(k + j) % 3]
            g = (16, 8, 32)[(k + j) % 3]
            R, qp = (8, 15)[(k + j) % 2], SAO_QPS[(k + 2 * j) % 3]
            out.append(inter_case(f"{kind}{g}-{w}x{h}-{bd}bit-R{R}-qp{qp}", w, h, bd, R, qp, f"{kind}{g}", seed=50 + 2 * k + j, noise=(k + j) % 3 << (bd - 8), rdo_zero=(k + j) & 1,
                                  centres=None if k else ((2, -1), (-4, 2))))
    out.append(inter_case("b-same16-64x64-8bit-lam0", 64, 64, 8, 8, 27, "b-same16", seed=61, lam=(0, 60)))
    out.append(inter_case("b-mix16-136x72-8bit-lam0", 136, 72, 8, 8, 27, "b-mix16", seed=62, noise=1, lam=(0, 60), rdo_zero=1))
    # low-contrast anchors + noise: the costs of a ring's candidates, of a node and its four children, of the three B keys lie a few units of SATD apart, so these are the
    # cases in which HOW the SATD is rounded decides (per 8x8 tile, not once per CU: SATD_ROUNDING_CASES; seeds and noise chosen so that the model itself says so)
    for kind, (w, h), bd, R, qp, noise, seed in (("soft-warp16", (136, 72), 8, 8, 32, 2, 203), ("soft-b-mix16", (136, 72), 8, 8, 32, 2, 201), ("soft-warp32", (64, 64), 8, 15, 22, 5, 200),
                                                 ("soft-b-mix16", (64, 64), 10, 8, 32, 5, 204), ("soft-warp16", (72, 104), 8, 8, 32, 5, 202), ("soft-b-mix32", (72, 104), 8, 15, 22, 3, 201),
                                                 ("soft-warp16", (136, 72), 10, 8, 32, 5, 200)):
        out.append(inter_case(f"{kind}-{w}x{h}-{bd}bit-R{R}-qp{qp}-n{noise}", w, h, bd, R, qp, kind, seed=seed, noise=noise << (bd - 8), rdo_zero=seed & 1))
    # rdo_cg > 0: these two pictures carry almost no residual (6 and 27 coded groups); the residual-rich ones follow
    out.append(inter_case("rdocg-warp16-136x72-8bit", 136, 72, 8, 8, 32, "warp16", seed=90, noise=2, rdo_zero=1, rdo_cg=5))
    out.append(inter_case("rdocg-b-mix16-72x104-10bit", 72, 104, 10, 8, 32, "b-mix16", seed=91, noise=4, rdo_zero=1, rdo_cg=5))
    # B pictures in which one CU's list-1 key EQUALS its bi-prediction key with list 0 dearer: 16 (SATD_1 - SATD_bi) = lambda_sad_q4 (mv_bits_0 - 1); found with the model
    # alone (tools/find_b_key_tie.py): what holds the order of list 1 against both lists on equal cost
    out.append(inter_case("b-tie12-b-mix8-64x64-8bit-lam16", 64, 64, 8, 8, 27, "b-mix8", seed=302, noise=3, lam=(16, None)))
    out.append(inter_case("b-tie12-b-mix8-136x72-10bit-lam32", 136, 72, 10, 8, 27, "b-mix8", seed=300, noise=1 << 2, lam=(32, None)))
    # residual-rich pictures: noise of +-6 .. 8 at QP 22 / 27 leaves hundreds of coded 4x4 groups, so that the group drop (rdo_cg), the TU zero-out and the
    # estimate work on real levels; each picture once with its rdo_cg and once at rdo_cg = 0 with the TU zero-out on
    for (w, h), bd, qp, content, seed, noise, cg, rz in RICH_PICTURES:
        out.append(inter_case(f"rich-{content}-{w}x{h}-{bd}bit-qp{qp}-s{seed}-cg{cg}-rz{rz}", w, h, bd, 8, qp, content, seed=seed, noise=noise << (bd - 8), rdo_zero=rz, rdo_cg=cg))
        out.append(inter_case(f"rich-{content}-{w}x{h}-{bd}bit-qp{qp}-s{seed}-cg0-rz1", w, h, bd, 8, qp, content, seed=seed, noise=noise << (bd - 8), rdo_zero=1))
    assert len({c.id for c in out}) == len(out)
    return out


RICH_PICTURES = (((136, 72), 8, 22, "warp8", 5, 6, 2, 1), ((72, 104), 10, 22, "warp16", 5, 6, 5, 1), ((64, 64), 8, 22, "warp32", 5, 8, 8, 0), ((64, 64), 10, 27, "warp8", 6, 7, 5, 1),
                 ((136, 72), 10, 27, "warp16", 7, 6, 2, 0), ((72, 104), 8, 27, "warp32", 8, 8, 5, 1), ((64, 64), 8, 27, "warp16", 9, 7, 2, 1), ((136, 72), 10, 22, "warp32", 10, 8, 5, 0),
                 ((72, 104), 8, 22, "warp8", 11, 6, 8, 1), ((64, 64), 10, 22, "warp16", 5, 6, 8, 1), ((136, 72), 8, 27, "warp32", 12, 7, 8, 0), ((72, 104), 10, 27, "warp8", 13, 8, 2, 1),
                 ((136, 72), 8, 22, "b-mix16", 14, 6, 5, 1), ((72, 104), 10, 22, "warp32", 15, 7, 2, 0), ((64, 64), 8, 22, "warp8", 16, 8, 5, 0), ((64, 64), 10, 22, "warp32", 17, 6, 5, 1))
INTER_CASES = _inter_cases()
RICH_CASES = [c for c in INTER_CASES if c.id.startswith("rich-")]
# the four of them that also run with sign data hiding, on the CPU against the stepped kernels: 8 and 10 bit, P and B, rdo_cg 5 and 0
SIGN_HIDE_CASES = [c for c in RICH_CASES if c.id in ("rich-b-mix16-136x72-8bit-qp22-s14-cg5-rz1", "rich-b-mix16-136x72-8bit-qp22-s14-cg0-rz1",
                                                     "rich-warp16-72x104-10bit-qp22-s5-cg5-rz1", "rich-warp32-136x72-10bit-qp22-s10-cg0-rz1")]
assert len(SIGN_HIDE_CASES) == 4
SATD_ROUNDING_CASES = [c for c in INTER_CASES if c.content.startswith("soft-")]


def inter_diff(want, got):
    """want: the model's Result; got: an O.Analysis of the oracle, the stepped kernel or the device.  '' when equal"""
    out = []
    a, b = want.cu, got.cu
    for f in a.dtype.names:
        if not np.array_equal(a[f], b[f]):
            i = tuple(np.argwhere(a[f] != b[f])[0][:2])
            out.append(f"cu.{f} at (row, column) {i}: model {a[i]} vs {b[i]}")
    for n, p, q in (("coef_y", want.coef[0], got.coef_y), ("coef_u", want.coef[1], got.coef_u), ("coef_v", want.coef[2], got.coef_v),
                    ("rec.y", want.rec[0], got.rec.y), ("rec.u", want.rec[1], got.rec.u), ("rec.v", want.rec[2], got.rec.v)):
        if not np.array_equal(p, q):
            ys, xs = np.nonzero(np.asarray(p) != np.asarray(q))
            out.append(f"{n}: {len(ys)} differ, first at x={xs[0]} y={ys[0]}: model {p[ys[0], xs[0]]} vs {q[ys[0], xs[0]]}")
    if want.est != got.est:
        out.append(f"estimate: model {want.est} vs {got.est}")
    return "; ".join(out)


def run_inter_case(api_or_oracle, c):
    """the case through the oracle module or a StageApi, with the centres the case gives (None with the pre-search: the entry makes its own)"""
    prm, cp = inter_case_params(c)
    cur, refs, _ = inter_case_pictures(c)
    cen = inter_case_centres(c, len(refs))
    if api_or_oracle is O:
        return O.analyze_inter(cur, refs[0], prm, cen[0], dump_me=True) if len(refs) == 1 else O.analyze_b(cur, refs[0], refs[1], prm, cen[0], cen[1], dump_me=True)
    return api_or_oracle.inter(cur, refs[0], cp, cen[0]) if len(refs) == 1 else api_or_oracle.b(cur, refs[0], refs[1], cp, cen[0], cen[1])


# hand-worked pictures of the inter audit (64x64, me_range 8, QP 27, no noise: every planted block is matched exactly); the device file runs them too
PIN_MVS, PIN_B_MVS = ((13, -9), (0, 0), (14, -8), (0, 0), (-2, 6), (0, 0), (7, -3), (0, 0)), ((5, 2), (-3, 6))      # quarter, half in x, half in both, quarter
PIN_SPLIT_MVS = ((4, 0), (0, 0), (-8, 4), (0, 0), (2, -4), (0, 0), (0, 6), (0, 0), (-5, -5), (0, 0), (7, 1), (0, 0), (-12, 9))    # block i of a P picture takes entry 2 i mod 13
INTER_PINS = {c.id: c for c in (
    inter_case("pin-flat", 64, 64, 8, 8, 27, "flat"),
    inter_case("pin-planted", 64, 64, 8, 8, 27, "warp32", mvs=PIN_MVS),
    inter_case("pin-split", 64, 64, 8, 8, 27, "warp16", mvs=PIN_SPLIT_MVS),
    inter_case("pin-main10", 64, 64, 10, 8, 27, "warp32", mvs=PIN_MVS),
    inter_case("pin-b-both", 64, 64, 8, 8, 27, "b-avg32", mvs=PIN_B_MVS),
    inter_case("pin-b-list0", 64, 64, 8, 8, 27, "b-first32", mvs=PIN_B_MVS),
    inter_case("pin-b-list1", 64, 64, 8, 8, 27, "b-second32", mvs=PIN_B_MVS))}


# hand-worked coefficient-group drops (rdo_cg = 2: the group's lambda is lambda_q4 itself): every block is matched exactly, one block carries a planted residual.
# GROUP_PINS[name]: the planted block (plane, x, y, n, dc, e), QP, and the lambda_q4 at which 16 D EQUALS the threshold of the DC group; the cases run at that lambda_q4,
# one below and one above
GROUP_PINS = {"8x8-8bit": (8, "warp8", PIN_SPLIT_MVS, (0, 16, 16, 8, 4, 0), 32, 1428), "8x8-10bit": (10, "warp8", PIN_SPLIT_MVS, (0, 16, 16, 8, 8, 0), 24, 5120),
              "32x32-8bit": (8, "warp32", PIN_MVS, (0, 32, 0, 32, 1, 0), 32, 1428), "32x32-10bit": (10, "warp32", PIN_MVS, (0, 32, 0, 32, 2, 0), 24, 5120)}
for _name, (_bd, _content, _mvs, _plant, _qp, _lq) in GROUP_PINS.items():
    for _step, _tag in ((-1, "below"), (0, "equal"), (1, "above")):
        INTER_PINS[f"pin-cg-{_name}-{_tag}"] = inter_case(f"pin-cg-{_name}-{_tag}", 64, 64, _bd, 8, _qp, _content, mvs=_mvs, rdo_cg=2, lam=(None, _lq + _step), plant=(_plant,))
# two groups in one 8x8 TU, (0, 0) and (1, 0): at lambda_q4 = 1500 the first goes and the second stays
INTER_PINS["pin-cg-one-of-two"] = inter_case("pin-cg-one-of-two", 64, 64, 8, 8, 32, "warp8", mvs=PIN_SPLIT_MVS, rdo_cg=2, lam=(None, 1500), plant=((0, 16, 16, 8, 4, 8),))


# ================================================================ the scene-cut sums (mihevc_k_scene_diff; tests/scene_ref.py is the reference)
def scene_diff(lib, planes, width, height, bit_depth, device=0, pitches=None):
    """planes: n 2-D arrays (uint8 at 8 bit, uint16 at 10), each of `height` rows; a plane's row length is its pitch -> (return code, [n sums])"""
    import ctypes as C
    n = len(planes)
    keep = [np.ascontiguousarray(p) for p in planes]
    ptrs = (C.c_void_p * max(n, 1))(*[p.ctypes.data for p in keep])
    pitch = (C.c_int32 * max(n, 1))(*(pitches if pitches is not None else [p.shape[1] for p in keep]))
    out = (C.c_uint64 * max(n, 1))(*([0xdeadbeef] * max(n, 1)))
    rc = lib.mihevc_k_scene_diff(device, ptrs, pitch, n, width, height, bit_depth, out)
    return rc, list(out)[:n]
