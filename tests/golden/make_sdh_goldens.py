#!/usr/bin/env python3
"""Golden coded pictures with sign data hiding (cfg.sign_hide = 1): `python tests/golden/make_sdh_goldens.py` rewrites tests/golden/streams_sdh.json.

The cases of make_stream_goldens.py with sign_hide = 1, plus one with B pictures.  The oracle has no sign data hiding, so here the KERNEL SOURCES
stepped on the CPU with the switch on (tests/emu) analyse every picture, in the order and with the parameters a session uses, the product's
host coder turns the symbols into slice NAL units, and the SHA-256 of every coded picture (decoding order) and of every reconstruction (display
order) goes into the fixture.  tests/test_sign_hiding_cpu.py recomputes them and decodes them with the repository's decoder (whose sign inference
was written apart from the encoder); tests/test_gpu_sign_hiding.py checks that an MI355X session produces the same bytes."""
import ctypes as C
import hashlib
import importlib.util
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from hevc_amd import _lib                 # noqa: E402
from oracle import oracle as O            # noqa: E402
from tests import util                    # noqa: E402

_spec = importlib.util.spec_from_file_location("make_stream_goldens", Path(__file__).parent / "make_stream_goldens.py")
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

CASES = dict(G.CASES)
CASES["b96x80_bframes"] = (96, 80, 8, 7, 7, 1, 28, 8, 93, {"bframes": 1, "rdo_cg": 5})
sha, frame_hash = G.sha, G.frame_hash


def config(name):
    w, h, bd, n, keyint, lanes, qp, rng, level, extra = CASES[name]
    cfg = _lib.default_config()
    cfg.width, cfg.height, cfg.bit_depth, cfg.keyint, cfg.min_keyint, cfg.gops_in_flight = w, h, bd, keyint, 1, lanes
    cfg.qp, cfg.me_range, cfg.level_idc, cfg.scenecut, cfg.aud, cfg.hrd = qp, rng, level, 0, 0, 0
    for k, v in extra.items():
        setattr(cfg, k, v)
    cfg.sign_hide = 1
    return cfg


def frames(name):
    w, h, bd, n = CASES[name][:4]
    return [util.synth_frame(h, w, seed=77, shift=(2 * i, i // 2), bit_depth=bd) for i in range(n)]


def coding_order(n, with_b):
    """display positions of a closed GOP of n pictures in decoding order with their slice types (cfg.bframes = 1: I0 P2 b1 P4 b3 ...)"""
    if not with_b:
        return [(p, 1 if p else 2) for p in range(n)]
    anchors = list(range(0, n, 2)) + ([n - 1] if n > 1 and (n - 1) % 2 else [])
    out = [(0, 2)]
    for prev, cur in zip(anchors, anchors[1:]):
        out.append((cur, 1))
        if cur - prev == 2:
            out.append((prev + 1, 0))
    return out


def params(cfg, qp, idr):
    """the cost parameters a session hands its kernels for one picture (mihevc_cost_params; the stepped entries take sign_hide beside it)"""
    cp = _lib.cost_params(qp, cfg.bit_depth, cfg.me_range if cfg.me_range > 0 else 15)
    cp.tile_cols, cp.tile_rows = _lib.tile_grid(cfg) if idr else _lib.p_tile_grid(cfg)
    cp.intra_nxn, cp.intra_in_p, cp.pre_search, cp.rdo_zero, cp.chroma_modes = cfg.intra_nxn, cfg.intra_in_p, cfg.pre_search, cfg.rdo_zero, cfg.chroma_modes
    cp.rdo_cg = max(0, cfg.rdo_cg)
    return cp


def stepped_pictures(api, cfg, srcs, idr, qp):
    """the session's pipeline, stepped: [(display position, slice type, coded picture bytes, analysis, reconstruction after the loop filters)] in
    decoding order.  idr: display positions of the IDR pictures; qp: the P pictures' QP (IDR qp - 3, B qp + 2, as a fixed-QP session)."""
    lib = _lib.load()
    bd, (w, h) = cfg.bit_depth, (cfg.width, cfg.height)
    cw, ch = (w + 7) & ~7, (h + 7) & ~7
    pads = [O.Frame(np.pad(f.y, ((0, ch - h), (0, cw - w)), mode="edge"), np.pad(f.u, ((0, (ch - h) // 2), (0, (cw - w) // 2)), mode="edge"),
                    np.pad(f.v, ((0, (ch - h) // 2), (0, (cw - w) // 2)), mode="edge")) for f in srcs]
    buf = (C.c_uint8 * (4 << 20))()
    out = []
    for g0, g1 in zip(idr, idr[1:] + [len(srcs)]):
        rec, last = {}, None
        for pos, st in coding_order(g1 - g0, cfg.bframes > 0):
            i, src = g0 + pos, pads[g0 + pos]
            cp = params(cfg, max(0, qp - 3) if st == 2 else qp + 2 if st == 0 else qp, st == 2)
            cen = (lambda other: O.search_centres(src, pads[other], bd) if cfg.pre_search else None)
            if st == 2:
                a = api.intra(src, cp)
            elif st == 1:
                a = api.inter(src, rec[last], cp, centers=cen(g0 + last if cfg.bframes > 0 else i - 1))
            else:
                a = api.b(src, rec[pos - 1], rec[pos + 1], cp, cen(i - 1), cen(i + 1))
            rec[pos], sao = O.sao(src, O.deblock(a.rec, a.cu, bd), cp)
            if st != 0:
                last = pos
            nb = lib.mihevc_encode_picture_host(C.byref(cfg), st, pos, cp.qp, util.ptr(a.cu), util.ptr(a.coef_y), util.ptr(a.coef_u), util.ptr(a.coef_v),
                                                util.ptr(sao), buf, len(buf))
            assert nb > 0, (nb, lib.mihevc_last_error(None))
            out.append((i, st, bytes(buf[:nb]), a, rec[pos]))
    return out


def case_pictures(name, api=None):
    w, h, bd, n, keyint, lanes, qp = CASES[name][:7]
    return stepped_pictures(api or util.StageApi(util.stepped_library(), "emu_", sign_hide=1), config(name), frames(name), util.idr_positions(n, keyint, lanes), qp)


def summary(pics):
    recon = dict((i, r) for i, _, _, _, r in pics)
    return {"pictures": [sha(p) for _, _, p, _, _ in pics], "bytes": [len(p) for _, _, p, _, _ in pics], "recon": [frame_hash(recon[i]) for i in sorted(recon)]}


if __name__ == "__main__":
    api = util.StageApi(util.stepped_library(), "emu_", sign_hide=1)
    out = {name: summary(case_pictures(name, api)) for name in CASES}
    (Path(__file__).parent / "streams_sdh.json").write_text(json.dumps(out, indent=1) + "\n")
    for k, v in out.items():
        print(k, v["bytes"])
