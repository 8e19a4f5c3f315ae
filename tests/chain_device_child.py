"""Child process of tests/test_gpu_chain.py (not a test): the route that holds the frames in torch tensors.  torch's bundled HIP runtime finds no device once the
library's is up, and in a pytest process the library comes up while the test files are collected; here torch comes first.  Feeds the clips of
two cases from device planes through Encoder.send_chain, the full chain (the planes are copied into the first ring) and a chain that begins with its resize stage
(the kernel reads them where they lie), and prints one JSON object with the SHA-256 of every stream and its pts list; the parent holds them against its model-fed
sessions."""
import hashlib
import json
import sys

import torch

torch.cuda.init()                                        # before the first mihevc_* call

from hevc_amd.encoder import Encoder                     # noqa: E402
from tests import chain_common as K                      # noqa: E402
from tests.ingest_common import device_planes            # noqa: E402


def main():
    out = {}
    for name in ("full", "upscale-interp3"):
        kind, size, chain = K.MULTI[name]
        for depth in (8, 10):
            keep = []
            with Encoder(K.cfg_of(depth, K.session_size((kind, size, chain))), device=0) as enc:
                enc.set_chain(*size, depth, **K.lib_kwargs(chain))
                for src in K.clip(kind, size, depth):
                    keep.append(device_planes(src))
                    enc.send_chain(*keep[-1])
                enc.flush()
                got = list(enc.packets())
            out[f"{name}-{depth}"] = [hashlib.sha256(b"".join(d for d, _, _ in got)).hexdigest(), [p for _, p, _ in got]]
    json.dump(out, sys.stdout)


if __name__ == "__main__":
    main()
