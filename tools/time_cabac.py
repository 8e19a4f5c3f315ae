#!/usr/bin/env python3
"""Time the host coder on ONE P picture, on the CPU: what a CABAC job of a session costs (the host tail).

  python tools/time_cabac.py [--width 1920 --height 1080 --repeats 50 --threads 1 --qp 27]

The symbols are the oracle's (oracle/oracle.py, as cpu_baseline in bench.py makes them): picture 0 of the synthetic `motion` clip analysed as an IDR
picture, picture 1 as a P picture against its filtered reconstruction, with the session's default knobs.  mihevc_encode_picture_host then codes the P
picture `repeats` times per thread (`threads` callers at once: the session's CABAC workers run side by side, and ctypes lets go of the interpreter
lock); the figures are the median, the fastest and the slowest call and the quartiles, in ms, over all calls.  The bytes of every call are compared with
the first call's.  Needs no GPU.  MIHEVC_LIBRARY selects the build (hevc_amd/_lib.py)."""
import argparse
import ctypes as C
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


class Picture:
    """the symbols of one P picture and what mihevc_encode_picture_host needs beside them"""

    def __init__(self, width, height, qp=27, me_range=0):
        from hevc_amd import _lib
        from hevc_amd.yuvio import SyntheticClip
        from oracle import oracle as O
        self.lib = _lib.load()
        cfg = self.cfg = _lib.default_config()
        cfg.width, cfg.height = width, height
        ch = (height + 7) & ~7
        clip = SyntheticClip("motion", 0, width, height, 2)
        frames = []
        for i in range(2):
            y, u, v = clip.frame(i)
            frames.append(O.Frame(np.pad(y, ((0, ch - height), (0, 0)), mode="edge"), np.pad(u, ((0, (ch - height) // 2), (0, 0)), mode="edge"),
                                  np.pad(v, ((0, (ch - height) // 2), (0, 0)), mode="edge")))
        prm_i, prm_p = O.default_params(max(0, qp - 3), me_range=me_range or 15), O.default_params(qp, me_range=me_range or 15)
        prm_i.tile_cols, prm_i.tile_rows = _lib.tile_grid(cfg)
        prm_i.intra_nxn, prm_i.chroma_modes = cfg.intra_nxn, cfg.chroma_modes
        prm_p.intra_in_p, prm_p.pre_search, prm_p.rdo_zero, prm_p.rdo_cg = cfg.intra_in_p, cfg.pre_search, cfg.rdo_zero, cfg.rdo_cg
        a = O.analyze_intra(frames[0], prm_i)
        ref, _ = O.sao(frames[0], O.deblock(a.rec, a.cu, 8), prm_i)
        cen = O.search_centres(frames[1], frames[0], 8) if cfg.pre_search else None
        self.analysis = O.analyze_inter(frames[1], ref, prm_p, centers=cen)
        _, self.sao = O.sao(frames[1], O.deblock(self.analysis.rec, self.analysis.cu, 8), prm_p)
        self.qp = prm_p.qp

    def call(self, buf):
        """one call into buf -> the access unit's size"""
        a = self.analysis
        n = self.lib.mihevc_encode_picture_host(C.byref(self.cfg), 1, 1, self.qp, a.cu.ctypes.data, a.coef_y.ctypes.data, a.coef_u.ctypes.data, a.coef_v.ctypes.data,
                                                self.sao.ctypes.data, buf, len(buf))
        if n < 0:
            raise RuntimeError(f"mihevc_encode_picture_host: {n} {self.lib.mihevc_last_error(None).decode()}")
        return n

    def encode(self):
        """one call -> the access unit's bytes"""
        buf = (C.c_uint8 * (8 << 20))()
        return C.string_at(buf, self.call(buf))

    def time(self, repeats, threads=1):
        """(seconds of every call, the bytes): `threads` callers at once, `repeats` calls each behind one warm-up call; the clock runs around the call alone"""
        want = self.encode()

        def caller(_):
            buf = (C.c_uint8 * (8 << 20))()
            self.call(buf)
            out = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                n = self.call(buf)
                out.append(time.perf_counter() - t0)
                if C.string_at(buf, n) != want:
                    raise RuntimeError("the coder's bytes changed between two calls")
            return out
        with ThreadPoolExecutor(max_workers=threads) as ex:
            times = [t for ts in ex.map(caller, range(threads)) for t in ts]
        return times, want


def summary(times):
    ms = sorted(t * 1e3 for t in times)
    q = statistics.quantiles(ms, n=4) if len(ms) > 1 else [ms[0]] * 3
    return {"calls": len(ms), "median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=27)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--threads", type=int, default=1)
    args = ap.parse_args(argv)
    pic = Picture(args.width, args.height, args.qp)
    times, data = pic.time(args.repeats, args.threads)
    s = summary(times)
    import json
    print(json.dumps({"picture": f"{args.width}x{args.height} P, qp {pic.qp}", "bytes": len(data), "threads": args.threads, **s}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
