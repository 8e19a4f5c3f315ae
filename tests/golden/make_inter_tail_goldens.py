#!/usr/bin/env python3
"""Golden coded pictures of one short session with sign data hiding: `python tests/golden/make_inter_tail_goldens.py` rewrites
tests/golden/streams_inter_tail.json.

12 pictures of 136x72 (partial CTUs on the right and at the bottom), keyint 6, two GOP lanes, sign_hide 1, made the way make_sdh_goldens.py makes its
cases (the kernel sources stepped on the CPU analyse every picture as a session would, the host coder writes the slices).  The fixture was written by the
commit BEFORE the inter CTU program's tail stages went from samples to 2x4 blocks; tests/test_inter_tail_cpu.py requires the stepped sources, and
tests/test_gpu_inter_tail.py an MI355X session, to produce the same bytes still."""
import importlib.util
import json
from pathlib import Path

HERE = Path(__file__).parent
NAME = "p136x72_two_lanes_sdh"
# width, height, bit depth, pictures, keyint, lanes, qp, me range, level, extra config knobs
CASE = (136, 72, 8, 12, 6, 2, 27, 8, 93, {})


def helper():
    """make_sdh_goldens.py, a private instance with this one case"""
    spec = importlib.util.spec_from_file_location("make_sdh_goldens_inter_tail", HERE / "make_sdh_goldens.py")
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    S.CASES = {NAME: CASE}
    return S


def compute():
    S = helper()
    return S.summary(S.case_pictures(NAME))


if __name__ == "__main__":
    out = {NAME: compute()}
    (HERE / "streams_inter_tail.json").write_text(json.dumps(out, indent=1) + "\n")
    print(NAME, out[NAME]["bytes"])
