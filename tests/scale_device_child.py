"""Child process of tests/test_gpu_scale.py (not a test): the routes that hold source planes in torch tensors.  torch's bundled HIP runtime finds no device
once the library's is up, and in a pytest process the library comes up while the test files are collected; here torch comes first.  Feeds
every source of the session tests from device planes through Encoder.send_scaled, then two sessions of different sizes from the same planes, and prints one
JSON object with the SHA-256 of every stream; the parent holds them against its model-fed sessions."""
import hashlib
import json
import sys

import torch

torch.cuda.init()                                        # before the first mihevc_* call

from hevc_amd.encoder import Encoder                     # noqa: E402
from tests.ingest_common import device_planes, drain     # noqa: E402
from tests.scale_common import OTHER, SOURCES, cfg_of, clip      # noqa: E402


def sha(b):
    return hashlib.sha256(b).hexdigest()


def main():
    out = {}
    for size in SOURCES:
        for depth in (8, 10):
            keep = []
            with Encoder(cfg_of(depth), device=0) as enc:
                for src in clip(size, depth):
                    keep.append(device_planes(src))
                    enc.send_scaled(size[0], size[1], *keep[-1])
                out[f"{size[0]}x{size[1]}-{depth}"] = sha(drain(enc))
    size, depth = SOURCES[0], 8
    frames = [device_planes(src) for src in clip(size, depth)]
    with Encoder(cfg_of(depth), device=0) as a, Encoder(cfg_of(depth, *OTHER), device=0) as b:
        for src in frames:
            a.send_scaled(size[0], size[1], *src)
            b.send_scaled(size[0], size[1], *src)
        out["two"] = [sha(drain(a)), sha(drain(b))]
    json.dump(out, sys.stdout)


if __name__ == "__main__":
    main()
