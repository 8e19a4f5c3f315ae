#!/usr/bin/env python3
"""What a session's FIRST chunk decides under rate control: `python tests/golden/make_step0_goldens.py` rewrites tests/golden/step0_estimates.json (needs an MI355X).

Step 0 of a chunk reads every lane's rate estimate back from the device and decides the IDR QPs from them (hevc_amd/csrc/session.cpp idr_step, rho_trial;
csrc/ratectl.h): one analysis, in a session's first chunk the rho trial, and a second analysis of the lanes whose wanted QP is far from the first one's.  The
fixture holds, per case, how many IDR analyses ran (mihevc_stats.stage_launches[0] with profile_stages 1) and the QP, type and coded size of every picture.  It
was written by the commit BEFORE the estimates went from one blocking copy per lane to queued copies behind one wait; tests/test_gpu_step0_estimates.py
requires a session to decide the same still.  `--scan` prints the same figures for a grid of inputs and writes nothing: how the cases were chosen."""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).parent
ROOT = HERE.parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

W, H, KEYINT = 256, 128, 4
# name: (content, pictures, gops_in_flight, crf, vbv_maxrate_kbps, vbv_bufsize_kbits, IDR analyses)
CASES = {
    "flat_no_redo": ("flat", 16, 4, 20, 16, 19, 1),          # the cap happens to ask for the QP the first analysis ran at
    "noise_redo": ("noise", 16, 4, 20, 1600, 1920, 2),       # a tenth of what white noise takes at CRF 20: every lane is analysed again, 13 QP steps up
    "single_lane": ("noise", 4, 1, 20, 1600, 1920, 2),
}


def picture(content, i):
    """picture i of a clip as three uint8 planes.  flat: a shallow ramp that creeps one sample a picture, grey chroma; noise: white noise, new in every picture"""
    yy, xx = np.mgrid[0:H, 0:W]
    if content == "flat":
        y = 96 + (xx + yy + 4 * i) // 16
        u = v = np.full((H // 2, W // 2), 128)
    else:
        rng = np.random.default_rng(1000 + i)
        y, u, v = rng.integers(0, 256, (H, W)), rng.integers(0, 256, (H // 2, W // 2)), rng.integers(0, 256, (H // 2, W // 2))
    return [np.ascontiguousarray(p.astype(np.uint8)) for p in (y, u, v)]


def config(lanes, crf, maxrate, bufsize):
    from hevc_amd import _lib
    cfg = _lib.default_config()
    cfg.width, cfg.height, cfg.keyint, cfg.min_keyint, cfg.gops_in_flight, cfg.scenecut, cfg.me_range, cfg.level_idc = W, H, KEYINT, 2, lanes, 0, 8, 93
    cfg.crf, cfg.qp, cfg.vbv_maxrate_kbps, cfg.vbv_bufsize_kbits, cfg.profile_stages = crf, -1, maxrate, bufsize, 1
    return cfg


def run(content, n, lanes, crf, maxrate, bufsize):
    """one session over the clip -> the record of its (only) chunk"""
    from hevc_amd.encoder import Encoder
    with Encoder(config(lanes, crf, maxrate, bufsize), device=0) as enc:
        for i in range(n):
            enc.send(*picture(content, i))
        enc.flush()
        packets = list(enc.packets_dts())
        st = enc.stats()
        info = [enc.frame_info(i) for i in range(n)]
    assert len(packets) == n
    return {"idr_analyses": int(st.stage_launches[0]), "qp": [q for q, _, _ in info], "type": [t for _, t, _ in info], "bits": [int(b) for _, _, b in info],
            "packet_bytes": [len(p[0]) for p in packets], "pts": [p[1] for p in packets]}


def compute(name):
    content, n, lanes, crf, maxrate, bufsize, _ = CASES[name]
    return run(content, n, lanes, crf, maxrate, bufsize)


if __name__ == "__main__":
    if "--scan" in sys.argv:
        for content in ("flat", "noise"):
            for crf in (20, 30):
                for maxrate in (2, 4, 8, 12, 16, 24, 32, 48, 64, 100, 200, 400, 800, 1600):
                    for n, lanes in ((16, 4), (4, 1)):
                        r = run(content, n, lanes, crf, maxrate, maxrate * 6 // 5)
                        print(content, "crf", crf, "maxrate", maxrate, "lanes", lanes, "analyses", r["idr_analyses"], "qp", r["qp"], "bytes", r["packet_bytes"], flush=True)
        sys.exit(0)
    out = {}
    for name in CASES:
        out[name] = compute(name)
        assert out[name]["idr_analyses"] == CASES[name][6], (name, out[name]["idr_analyses"])
        print(name, out[name]["idr_analyses"], out[name]["qp"], sum(out[name]["packet_bytes"]))
    (HERE / "step0_estimates.json").write_text(json.dumps(out, indent=1) + "\n")
