"""Child process of tests/test_gpu_upscale.py (not a test): the route that holds source planes in torch tensors.  torch's bundled HIP runtime finds no device
once the library's is up, and in a pytest process the library comes up while the test files are collected; here torch comes first.  Feeds
every source of the session tests from device planes through Encoder.send_upscaled and prints one JSON object with the SHA-256 of every stream; the parent holds
them against its model-fed sessions."""
import hashlib
import json
import sys

import torch

torch.cuda.init()                                        # before the first mihevc_* call

from hevc_amd.encoder import Encoder                     # noqa: E402
from tests.ingest_common import device_planes, drain     # noqa: E402
from tests.upscale_common import SOURCES, cfg_of, clip   # noqa: E402


def main():
    out = {}
    for size in SOURCES:
        for depth in (8, 10):
            keep = []
            with Encoder(cfg_of(depth), device=0) as enc:
                for src in clip(size, depth):
                    keep.append(device_planes(src))
                    enc.send_upscaled(size[0], size[1], *keep[-1])
                out[f"{size[0]}x{size[1]}-{depth}"] = hashlib.sha256(drain(enc)).hexdigest()
    json.dump(out, sys.stdout)


if __name__ == "__main__":
    main()
