"""GPU (-m gpu): the streams of small sessions read back by the independent syntax reader (tests/hevc_syntax.py).  What it reads -- quadtree,
modes, motion, cbfs, levels, SAO, slice QP, NAL type and POC -- must equal, picture by picture, the analyses of the oracle pipeline replayed with the
session's QPs (the replay also asserts that the session's reconstruction equals the oracle's), and the samples tests/hevc_recon.py rebuilds from
what it reads must equal the session's reconstruction."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import hevc_recon as R
from tests import hevc_syntax as S
from tests import util
from tests.test_syntax_independent import check_parameter_sets, check_picture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


def small_cfg(w, h, bd, **kw):
    from hevc_amd import _lib
    cfg = _lib.default_config()
    cfg.width, cfg.height, cfg.bit_depth, cfg.keyint, cfg.min_keyint, cfg.me_range, cfg.gops_in_flight, cfg.aud = w, h, bd, 3, 2, 8, 2, 1
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def check_recon(st, recs):
    """the independent reconstruction of every picture equals the session's (recs by display position, at the coded size) and its hash SEI, if
    any; -> the reconstruction's coverage counter"""
    stats = {}
    out = R.reconstruct(st, stats)
    base = 0
    for k, (pic, (poc, y, u, v)) in enumerate(zip(st.pictures, out)):
        if pic.nal_type in (19, 20):
            base = k                                            # closed GOPs: an IDR's display position is its decoding position
        r = recs[base + poc]
        for c, (a, b) in enumerate(((y, r.y), (u, r.u), (v, r.v))):
            assert a.shape == b.shape and np.array_equal(a, b), \
                "display picture %d plane %d: %d samples of the session's reconstruction differ from the independent one" % (base + poc, c, int((a != b).sum()))
    for k, hh in enumerate(stats["hash"]):
        assert hh is None or hh[1] == hh[2], "picture %d: hash SEI %s, independent reconstruction %s" % (k, hh[1], hh[2])
    return stats["cov"]


def check_session(st, replayed, infos):
    """replayed: (analysis, SAO parameters, QP, slice type, display index) in decoding order"""
    idr = [i for i, (_, t, _) in enumerate(infos) if t == 2]
    assert len(st.pictures) == len(replayed)
    for pic, (a, sao, qp, stype, i) in zip(st.pictures, replayed):
        g0 = max(j for j in idr if j <= i)
        check_picture(pic, a, sao, qp, stype, {2: 19, 1: 1, 0: 0}[stype], i - g0)


@pytest.mark.parametrize("w,h,bd,qp,pre,content", [(96, 80, 8, 26, 1, "synth"), (96, 80, 8, 0, 1, "full_range"), (72, 104, 10, 51, 0, "full_range")])
def test_session_streams_read_independently_equal_the_replayed_analyses(lib, w, h, bd, qp, pre, content):
    from hevc_amd import _lib
    from tests.test_bitstream_cpu import flashing_clip
    from tests.test_gpu_configs import replay, run_session
    cfg = small_cfg(w, h, bd, qp=qp, pre_search=pre)
    n = 5
    srcs = [util.synth_frame(h, w, seed=3, shift=(3 * i, i), bit_depth=bd) for i in range(n)] if content == "synth" else flashing_clip(w, h, bd, n)
    frames = [(util.planes(f, bd), f) for f in srcs]
    stream, _, infos, recs, _ = run_session(cfg, frames)
    out = []
    replay(lib, cfg, frames, infos, recs, n, out=out)
    st = S.parse_stream(stream)
    check_session(st, out, infos)
    check_parameter_sets(st, cfg, (_lib.tile_grid(cfg), _lib.p_tile_grid(cfg)))
    check_recon(st, recs)


def test_session_with_p_tiles_read_independently(lib):
    from hevc_amd import _lib
    from tests.test_gpu_configs import replay, run_session
    w, h, bd = 512, 64, 8
    cfg = small_cfg(w, h, bd, qp=30, level_idc=120, p_tiles=1)
    assert _lib.p_tile_grid(cfg) == (2, 1) and _lib.tile_grid(cfg) == (2, 1)
    n = 4
    frames = [(util.planes(f, bd), f) for f in (util.synth_frame(h, w, seed=31, shift=(5 * i, 2 * i), bit_depth=bd) for i in range(n))]
    stream, _, infos, recs, _ = run_session(cfg, frames)
    out = []
    replay(lib, cfg, frames, infos, recs, n, out=out)
    st = S.parse_stream(stream)
    check_session(st, out, infos)
    check_parameter_sets(st, cfg, ((2, 1), (2, 1)))
    assert all(len(p.slices[0]["header"]["entry_point_offsets"]) == 1 for p in st.pictures)
    check_recon(st, recs)


def test_b_session_read_independently(lib):
    from hevc_amd import _lib
    from tests.test_gpu_bframes import replay, run_b_session
    w, h, bd, n = 72, 104, 10, 7
    cfg = small_cfg(w, h, bd, qp=28, bframes=1, keyint=7, scenecut=0, level_idc=93)
    frames = [util.synth_frame(h, w, seed=9, shift=(3 * i, i), bit_depth=bd) for i in range(n)]
    pk, infos, recs, _ = run_b_session(cfg, frames, bd)
    out = []
    replay(lib, cfg, frames, infos, recs, out=out)
    st = S.parse_stream(b"".join(p[0] for p in pk))
    check_session(st, out, infos)
    check_parameter_sets(st, cfg, (_lib.tile_grid(cfg), _lib.p_tile_grid(cfg)))
    assert check_recon(st, recs)["inter", "bi"] > 0
    kinds = set()
    for pic in st.pictures:
        if pic.slices[0]["slice_type"] == 0:
            inter = pic.cu["inter"] == 1
            kinds |= set(zip(pic.cu["pf0"][inter].tolist(), pic.cu["pf1"][inter].tolist()))
    assert kinds == {(1, 0), (0, 1), (1, 1)}, kinds


def test_sliced_encoder_stream_read_independently(lib):
    """two sessions, one band of CTU rows each, exchanging rows (cfg.slice_halo): the whole-picture pipeline of test_sliced_cpu.halo_pipeline is
    what the slices together must code"""
    from hevc_amd import _lib
    from hevc_amd.encoder import SlicedEncoder
    from tests.test_gpu_configs import session_params
    from tests.test_sliced_cpu import halo_pipeline
    w, h, bd, n = 160, 96, 8, 5
    cfg = small_cfg(w, h, bd, qp=27, level_idc=63, keyint=4, me_range=12)
    frames = [util.synth_frame(h, w, seed=5, shift=(2 * i, 7 * i), bit_depth=bd) for i in range(n)]
    sl = SlicedEncoder(cfg, [0, 0], keep_recon=True)
    try:
        got = []
        for f in frames:
            sl.send(*util.planes(f, bd))
            got += sl.ready()
        got += sl.finish()
        recs = [O.Frame(*sl.recon(i)) for i in range(n)]
        infos = [sl._encs[0].frame_info(i) for i in range(n)]
        cfgs, rows = sl._cfgs, sl.rows
    finally:
        sl.close()
    st = S.parse_stream(b"".join(d for d, _, _ in got))
    idr_at = {i for i, (_, t, _) in enumerate(infos) if t == 2}
    wc = (w + 31) >> 5
    pipe = halo_pipeline(frames, rows, cfgs, None, None, None, bd, prm_of=lambda i, intra: session_params(lib, cfgs[0], infos[i][0], False)[0], idr_at=idr_at)
    assert len(st.pictures) == n
    for i, (pic, (intra, a, sao, ref)) in enumerate(zip(st.pictures, pipe)):
        assert recs[i].same(ref)
        assert [s["address"] for s in pic.slices] == [sum(rows[:k]) * wc for k in range(len(rows))]
        g0 = max(j for j in idr_at if j <= i)
        check_picture(pic, a, sao, infos[i][0], 2 if intra else 1, 19 if intra else 1, i - g0)
    check_parameter_sets(st, cfgs[0], (_lib.tile_grid(cfgs[0]), _lib.p_tile_grid(cfgs[0])))
    assert np.all([len(p.slices) == len(rows) for p in st.pictures])
    check_recon(st, recs)
