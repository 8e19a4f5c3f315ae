"""Child process of tests/test_gpu_sr.py (not a test): the route that holds the source in torch tensors.  torch's bundled HIP runtime finds no device once the
library's is up, and in a pytest process the library comes up while the test files are collected; here torch comes first.  Feeds every clip
of the session tests through Encoder.send_sr from device planes and through Encoder.send_sr_tensor from one (3, H, W) tensor, and prints one JSON object with
the SHA-256 of every stream; the parent holds them against its own sessions."""
import hashlib
import json
import sys

import numpy as np
import torch

torch.cuda.init()                                        # before the first mihevc_* call

from hevc_amd.encoder import Encoder                     # noqa: E402
from tests import sr_common as S                         # noqa: E402
from tests.ingest_common import device_planes, drain     # noqa: E402


def main():
    out = {}
    for scale in (4, 2):
        for depth in (8, 10):
            fmt = S.session_format(depth)
            sw, sh = S.SESSION_W // scale, S.SESSION_H // scale
            keep = []
            with Encoder(S.session_cfg(depth), device=0) as enc:
                enc.set_sr_model(S.session_model(scale))
                for planes in S.session_clip(scale, depth):
                    keep.append(device_planes(planes))
                    enc.send_sr(fmt, sw, sh, *keep[-1])
                out[f"planes-x{scale}-{depth}"] = hashlib.sha256(drain(enc)).hexdigest()
            if depth > 8:          # send_sr_tensor reads a 16-bit tensor as a 16-bit source: a 10-bit clip through it would be another picture
                continue
            with Encoder(S.session_cfg(depth), device=0) as enc:
                enc.set_sr_model(S.session_model(scale))
                for g, b, r in S.session_clip(scale, depth):
                    keep.append(torch.from_numpy(np.stack([r, g, b])).cuda())
                    enc.send_sr_tensor(keep[-1])
                out[f"tensor-x{scale}-{depth}"] = hashlib.sha256(drain(enc)).hexdigest()
    json.dump(out, sys.stdout)


if __name__ == "__main__":
    main()
