"""CPU: the tail stages of the inter CTU program by 2x4 block (residual, RD zero-out, outputs), the TU descriptors at block origins only (all four
callers of residual_pipeline) and the integer-vector SATDs on lane pairs, stepped from the kernel sources (tests/emu) against the oracle.

Pictures whose CTUs are partial in both directions (whole blocks and tiles outside the picture), Main10, a low QP with many levels and small CUs; RD zero-out
on (TUs dropped and kept) and off with the coefficient-group zero-out; the intra second pass (the a.ip sums of the output stage); a B picture; an IDR picture
with tiles, NxN and chroma modes for the intra callers' descriptors.  The partial and the rich picture again with reversed / shuffled lanes and a pseudo-random
initial LDS: a block written by two lanes, or an entry read before it is written, shows there.

Sign data hiding: the oracle has none (oracle/ does not know the switch), so with sign_hide = 1 the reference is the repository's independent numpy model of the
inter CTU program (tests/hevc_inter_cu.py, sign_hide = 1) started from the oracle's integer-search dump; with sign_hide = 0 it is the oracle itself."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import util

SHAPES = {"72x40": (72, 40, 8, 8, 5), "72x104": (72, 104, 10, 8, 7), "160x96": (160, 96, 8, 12, 3)}      # width, height, bit depth, me range, seed
KNOBS = [(26, 1, 0), (35, 1, 0), (22, 0, 5)]                                                            # QP, rdo_zero, rdo_cg
CASES = [(s, *k) for s in ("72x40", "72x104") for k in KNOBS] + [("160x96", 14, 1, 0), ("160x96", 14, 0, 5)]


@pytest.fixture(scope="module")
def emu():
    return {sh: util.StageApi(util.stepped_library(), "emu_", sign_hide=sh) for sh in (0, 1)}


def params(shape, qp, rdo_zero, rdo_cg, **knobs):
    w, h, bd, rng, seed = SHAPES[shape]
    prm = O.default_params(qp, bit_depth=bd, me_range=rng)
    prm.rdo_zero, prm.rdo_cg = rdo_zero, rdo_cg
    for k, v in knobs.items():
        setattr(prm, k, v)
    return prm


@functools.lru_cache(maxsize=None)
def pictures(shape, qp):
    """(source of the P picture, its reference: the oracle's loop-filtered IDR picture)"""
    w, h, bd, rng, seed = SHAPES[shape]
    srcs = [util.synth_frame(h, w, seed=seed, shift=(3 * i, 2 * i), bit_depth=bd) for i in range(2)]
    prm_i = O.default_params(max(0, qp - 3), bit_depth=bd, me_range=rng)
    a = O.analyze_intra(srcs[0], prm_i)
    ref, _ = O.sao(srcs[0], O.deblock(a.rec, a.cu, bd), prm_i)
    return srcs[1], ref


@functools.lru_cache(maxsize=None)
def oracle_p(shape, qp, rdo_zero, rdo_cg):
    src, ref = pictures(shape, qp)
    return O.analyze_inter(src, ref, params(shape, qp, rdo_zero, rdo_cg), dump_me=True)


def aliasing(me):
    """(nodes of levels 0 / 1 whose vector a valid finer node over one of their tiles shares, those whose vector none shares): inter_tree's alias rule on the integer table"""
    yes = no = 0
    for ctu in me:
        for node, fine in [(0, range(1, 21))] + [(1 + q, range(5 + 4 * q, 9 + 4 * q)) for q in range(4)]:
            if ctu[node][2] < 0:
                continue
            shared = any(ctu[f][2] >= 0 and tuple(ctu[f][:2]) == tuple(ctu[node][:2]) for f in fine)
            yes, no = yes + shared, no + (not shared)
    return yes, no


def has_cbf(a):
    return bool((a.cu["flags"] & 14).any())


def test_the_cases_reach_what_they_are_for():
    """from the oracle alone: all three CU sizes, TUs dropped and TUs kept by the RD zero-out, nodes that alias a finer vector and nodes that do not"""
    sizes, yes, no = set(), 0, 0
    for shape, qp, rz, cg in CASES:
        a = oracle_p(shape, qp, rz, cg)
        sizes |= {int(v) for v in np.unique(a.cu["log2_size"][(a.cu["flags"] & 1) == 1])}
        y, n = aliasing(a.me)
        yes, no = yes + y, no + n
        if rz and qp >= 26:
            off = oracle_p(shape, qp, 0, cg)
            assert not util.same_analysis(a, off), (shape, qp, "the zero-out drops nothing")
            assert has_cbf(a), (shape, qp, "the zero-out drops everything")
    assert sizes == {3, 4, 5}, sizes
    assert yes > 0 and no > 0, (yes, no)


def check_p(api, shape, qp, rz, cg, sign_hide):
    src, ref = pictures(shape, qp)
    prm = params(shape, qp, rz, cg)
    want = oracle_p(shape, qp, rz, cg)
    got = api[sign_hide].inter(src, ref, prm)
    assert np.array_equal(want.me, got.me), "integer search"
    if not sign_hide:
        assert util.same_analysis(want, got), util.describe_diff(want, got)
        return
    model = model_p(shape, qp, rz, cg)
    assert util.inter_diff(model, got) == ""
    assert util.inter_diff(model, want) != "" or not has_cbf(want), "sign hiding changed nothing"


@functools.lru_cache(maxsize=None)
def model_p(shape, qp, rz, cg):
    from tests import hevc_inter_cu as M
    w, h, bd, rng, seed = SHAPES[shape]
    src, ref = pictures(shape, qp)
    prm = params(shape, qp, rz, cg)
    return M.analyse(util.planes3(src), [util.planes3(ref)], [oracle_p(shape, qp, rz, cg).me], bd, prm.qp, prm.qp_c, prm.lambda_sad_q4, prm.lambda_q4, rng, [None], rz, 0, 0,
                     None, rdo_cg=cg, sign_hide=1)


@pytest.mark.parametrize("sign_hide", [0, 1])
@pytest.mark.parametrize("shape,qp,rz,cg", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_stepped_p_pictures(emu, shape, qp, rz, cg, sign_hide):
    check_p(emu, shape, qp, rz, cg, sign_hide)


@pytest.mark.parametrize("order,fill", [("1", None), ("2", "11")])
@pytest.mark.parametrize("shape,qp,rz,cg", [("72x40", 26, 1, 0), ("160x96", 14, 1, 0)], ids=["72x40", "160x96"])
def test_any_lane_order_and_initial_lds(emu, monkeypatch, shape, qp, rz, cg, order, fill):
    monkeypatch.setenv("EMU_ORDER", order)
    if fill:
        monkeypatch.setenv("EMU_SHARED_FILL", fill)
    for sign_hide in (0, 1):
        check_p(emu, shape, qp, rz, cg, sign_hide)


def test_intra_second_pass_sums(emu):
    """intra_in_p: the output stage's squared error and estimate of every CTU decide which CTUs the second pass recodes as intra"""
    from tests.test_bitstream_cpu import occluded_clip
    w, h, bd = 136, 72, 8
    prm = O.default_params(26, bit_depth=bd, me_range=8)
    prm.intra_in_p, prm.rdo_zero, prm.chroma_modes = 1, 1, 1
    srcs = occluded_clip(w, h, bd)
    a = O.analyze_intra(srcs[0], prm)
    ref = O.sao(srcs[0], O.deblock(a.rec, a.cu, bd), prm)[0]
    want, got = O.analyze_inter(srcs[1], ref, prm, dump_me=True), emu[0].inter(srcs[1], ref, prm)
    inter = (want.cu["flags"] & 1) == 1
    assert inter.any() and not inter.all(), "the clip must leave CTUs of both kinds"
    assert np.array_equal(want.me, got.me) and util.same_analysis(want, got), util.describe_diff(want, got)


def test_b_picture(emu):
    shape, qp = "72x40", 26
    w, h, bd, rng, seed = SHAPES[shape]
    prm_i, prm_p, prm_b = O.default_params(qp - 3, bd, rng), params(shape, qp, 1, 0), params(shape, qp + 2, 1, 5)
    f = [util.synth_frame(h, w, seed=23, shift=(3 * i, 2 * i), bit_depth=bd) for i in range(3)]
    a0 = O.analyze_intra(f[0], prm_i)
    r0, _ = O.sao(f[0], O.deblock(a0.rec, a0.cu, bd), prm_i)
    a2 = O.analyze_inter(f[2], r0, prm_p)
    r2, _ = O.sao(f[2], O.deblock(a2.rec, a2.cu, bd), prm_p)
    want, got = O.analyze_b(f[1], r0, r2, prm_b, None, None, dump_me=True), emu[0].b(f[1], r0, r2, prm_b, None, None)
    assert np.array_equal(want.me[0], got.me[0]) and np.array_equal(want.me[1], got.me[1])
    assert util.same_analysis(want, got), util.describe_diff(want, got)
    assert has_cbf(want)


def test_idr_picture_with_tiles_nxn_and_chroma_modes(emu):
    """the intra callers' descriptors (the plan's cost estimate over the whole CTU, the coding of every CU over its region)"""
    prm = O.default_params(26, bit_depth=8)
    prm.tile_cols, prm.tile_rows, prm.intra_nxn, prm.chroma_modes = 2, 2, 1, 1
    src = util.synth_frame(160, 544, seed=9, bit_depth=8)
    want, got = O.analyze_intra(src, prm), emu[0].intra(src, prm)
    assert (want.cu["flags"] & 16).any() and len(np.unique(want.cu["log2_size"])) >= 2
    assert util.same_analysis(want, got), util.describe_diff(want, got)


def test_stepped_session_still_produces_the_golden_pictures():
    """tests/golden/streams_inter_tail.json: 12 pictures, two GOP lanes, sign data hiding, written by the commit before the tail stages went to blocks"""
    import importlib.util
    import json
    from pathlib import Path
    golden = Path(__file__).parent / "golden"
    spec = importlib.util.spec_from_file_location("make_inter_tail_goldens", golden / "make_inter_tail_goldens.py")
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    want = json.loads((golden / "streams_inter_tail.json").read_text())[G.NAME]
    got = G.compute()
    assert got["bytes"] == want["bytes"] and got["pictures"] == want["pictures"] and got["recon"] == want["recon"]
    assert len(want["bytes"]) == 12
