"""Child process of tests/test_gpu_mcfi.py (not a test): the route that holds the frames in torch tensors.  torch's bundled HIP runtime finds no device once the
library's is up, and in a pytest process the library comes up while the test files are collected; here torch comes first.  Feeds the clip of
the session tests from device planes through Encoder.send_interpolate, at factors 2 and 3, and prints one JSON object with the SHA-256 of every stream and its
pts list; the parent holds them against its model-fed sessions."""
import hashlib
import json
import sys

import torch

torch.cuda.init()                                        # before the first mihevc_* call

from hevc_amd.encoder import Encoder                     # noqa: E402
from tests.ingest_common import device_planes            # noqa: E402
from tests.mcfi_common import cfg_of, clip               # noqa: E402


def main():
    out = {}
    for depth in (8, 10):
        for f in (2, 3):
            keep = []
            with Encoder(cfg_of(depth), device=0) as enc:
                for src in clip(depth):
                    keep.append(device_planes(src))
                    enc.send_interpolate(*keep[-1], factor=f)
                enc.flush()
                got = list(enc.packets())
            out[f"{depth}-{f}"] = [hashlib.sha256(b"".join(d for d, _, _ in got)).hexdigest(), [p for _, p, _ in got]]
    json.dump(out, sys.stdout)


if __name__ == "__main__":
    main()
