"""Child process of tests/test_gpu_lut3d.py (not a test): the route that holds the source frames in torch tensors.  torch's bundled HIP runtime finds no device once
the library's is up, and in a pytest process the library comes up while the test files are collected; here torch comes first.  Feeds the
clip of the session tests from device planes through Encoder.send_lut3d with MIHEVC_SRC_ASYNC, under one table and with the table replaced in the middle of the
clip without a sync in between, and prints one JSON object with the SHA-256 of every stream and its pts list; the parent holds them against its model-fed
sessions."""
import hashlib
import json
import sys

import torch

torch.cuda.init()                                        # before the first mihevc_* call

from hevc_amd.encoder import Encoder                     # noqa: E402
from tests.ingest_common import device_planes            # noqa: E402
from tests.lut3d_common import SRC_B, SRC_MATRIX, cfg_of, clip, session_table      # noqa: E402

PLANS = {"one": (0, 0, 0, 0, 0, 0, 0), "replaced": (0, 0, 0, 0, 1, 1, 1)}


def main():
    out = {}
    for depth in (8, 10):
        for name, plan in PLANS.items():
            keep, current = [], None
            with Encoder(cfg_of(depth), device=0) as enc:
                for src, which in zip(clip(), plan):
                    if which != current:
                        enc.set_lut3d(session_table(which))
                        current = which
                    keep.append(device_planes(src))
                    enc.send_lut3d(*keep[-1], bit_depth=SRC_B, matrix=SRC_MATRIX, asynchronous=True)
                enc.flush()
                got = list(enc.packets())
            out[f"{depth}-{name}"] = [hashlib.sha256(b"".join(d for d, _, _ in got)).hexdigest(), [p for _, p, _ in got]]
    json.dump(out, sys.stdout)


if __name__ == "__main__":
    main()
