"""Child process of tests/test_gpu_sr_yuv.py (not a test): the route that holds the source in torch tensors on the device.  torch's bundled HIP runtime finds no
device once the library's is up, and in a pytest process the library comes up while the test files are collected; here torch comes first.
Feeds the clips of the session tests through Encoder.send_sr_yuv and Encoder.send_sr_fit from device planes (MIHEVC_SRC_DEVICE), into a session of the
network's size and into a smaller one, and prints one JSON object with the SHA-256 of every stream; the parent holds them against its own sessions."""
import hashlib
import json
import sys

import torch

torch.cuda.init()                                        # before the first mihevc_* call

from hevc_amd.encoder import Encoder                     # noqa: E402
from tests import sr_common as S                         # noqa: E402
from tests import sr_yuv_common as Q                     # noqa: E402
from tests.ingest_common import device_planes            # noqa: E402


def main():
    out = {}
    for name, (w, h) in (("direct", (192, 128)), ("resized", (108, 72))):
        keep = []
        with Encoder(Q.session_cfg(8, w, h), device=0) as enc:
            enc.set_sr_model(S.session_model(4))
            for planes in Q.yuv_clip(48, 32, 8):
                keep.append(device_planes(planes))
                enc.send_sr_yuv(48, 32, *keep[-1], bit_depth=8, matrix=6)
            out[f"yuv-{name}"] = hashlib.sha256(Q.drain(enc)).hexdigest()
    with Encoder(Q.session_cfg(8, 108, 72), device=0) as enc:
        enc.set_sr_model(S.session_model(4))
        keep = []
        for planes in S.session_clip(4, 8):
            keep.append(device_planes(planes))
            enc.send_sr_fit(S.session_format(8), 48, 32, *keep[-1])
        out["fit-resized"] = hashlib.sha256(Q.drain(enc)).hexdigest()
    json.dump(out, sys.stdout)


if __name__ == "__main__":
    main()
