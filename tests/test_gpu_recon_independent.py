"""GPU (-m gpu): small sessions whose reconstruction on an MI355X must equal the one tests/hevc_recon.py rebuilds, independently of the kernels,
the oracle and the repository decoder, from the stream alone (tests/hevc_syntax.py), and whose decoded picture hash SEI must equal the hash of that
independent reconstruction.  They cover what the sessions of tests/test_gpu_syntax_independent.py do not: pictures whose coded size is not their
display size with content that pans out of the picture, Main 10 HDR10 with sign data hiding, every hash type, intra NxN and intra CUs in P
pictures, and slices that do not filter across their edges."""
import pytest

from oracle import oracle as O
from tests import hevc_syntax as S
from tests import util
from tests.test_gpu_syntax_independent import check_recon, small_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


def session(cfg, frames):
    from hevc_amd.encoder import Encoder
    bd = cfg.bit_depth
    with Encoder(cfg, device=0, keep_recon=True) as enc:
        for f in frames:
            enc.send(*util.planes(f, bd))
        enc.flush()
        stream = b"".join(d for d, _pts, _key in enc.packets())
        recs = [O.Frame(*enc.recon(i)) for i in range(len(frames))]
    return stream, recs


@pytest.mark.parametrize("w,h", [(322, 182), (100, 60)])
def test_off_grid_session_with_vectors_leaving_the_picture(lib, w, h):
    """coded size (w + 7) & ~7 by (h + 7) & ~7; the content pans by 6 and 3 samples a picture, so that blocks at the edges predict from beyond
    the coded picture (clamped reference positions)"""
    n = 4
    cfg = small_cfg(w, h, 8, qp=30, keyint=8)
    frames = [util.synth_frame(h, w, seed=41, shift=(6 * i, 3 * i)) for i in range(n)]
    stream, recs = session(cfg, frames)
    st = S.parse_stream(stream)
    assert (st.pictures[0].w, st.pictures[0].h) == ((w + 7) & ~7, (h + 7) & ~7) and recs[0].y.shape == (st.pictures[0].h, st.pictures[0].w)
    cov = check_recon(st, recs)
    assert cov["mc", "outside"] > 0 and cov["inter", "uni"] > 0


def test_hdr10_session_with_sign_hiding_and_md5(lib):
    w, h, bd, n = 96, 64, 10, 4
    cfg = small_cfg(w, h, bd, qp=26, keyint=8, sign_hide=1, pic_hash=1, hdr10=1, colour_primaries=9, transfer=16, matrix=9,
                    chroma_loc=0, level_idc=150)
    frames = [util.synth_frame(h, w, seed=43, shift=(3 * i, i), bit_depth=bd) for i in range(n)]
    stream, recs = session(cfg, frames)
    st = S.parse_stream(stream)
    assert all(st.pps[p.slices[0]["pps_id"]]["sign_data_hiding_enabled_flag"] == 1 for p in st.pictures)
    assert all(p.hash is not None and p.hash[0] == 0 for p in st.pictures)
    check_recon(st, recs)


@pytest.mark.parametrize("pic_hash", [2, 3])
def test_crc_and_checksum_sessions_with_nxn_and_intra_in_p(lib, pic_hash):
    w, h, bd, n = 136, 72, 8, 4
    cfg = small_cfg(w, h, bd, qp=28, keyint=8, pic_hash=pic_hash, intra_nxn=1, intra_in_p=1)
    from tests.test_bitstream_cpu import occluded_clip
    stream, recs = session(cfg, occluded_clip(w, h, bd, n))
    st = S.parse_stream(stream)
    assert all(p.hash is not None and p.hash[0] == pic_hash - 1 for p in st.pictures)
    check_recon(st, recs)


@pytest.mark.parametrize("w,h,bd", [(160, 96, 8), (96, 160, 10)])
def test_sliced_session_without_halo_stops_the_loop_filters_at_the_slice_edge(lib, w, h, bd):
    """cfg.slice_halo = 0: every band is coded as a slice with slice_loop_filter_across_slices_enabled_flag 0, so deblocking and SAO stop at the
    slice edges"""
    from hevc_amd.encoder import SlicedEncoder
    n = 3
    cfg = small_cfg(w, h, bd, qp=27, level_idc=63, keyint=4, me_range=12)
    frames = [util.synth_frame(h, w, seed=5, shift=(2 * i, 7 * i), bit_depth=bd) for i in range(n)]
    sl = SlicedEncoder(cfg, [0, 0], keep_recon=True, halo=False)
    rows = sl.rows
    try:
        got = []
        for f in frames:
            sl.send(*util.planes(f, bd))
            got += sl.ready()
        got += sl.finish()
        recs = [O.Frame(*sl.recon(i)) for i in range(n)]
    finally:
        sl.close()
    st = S.parse_stream(b"".join(d for d, _, _ in got))
    assert len(rows) == 2 and all(len(p.slices) == 2 for p in st.pictures)
    assert all(s["header"]["slice_loop_filter_across_slices_enabled_flag"] == 0 for p in st.pictures for s in p.slices[1:])
    cov = check_recon(st, recs)
    assert cov["deblock", "slice_edge_unfiltered"] > 0


def test_1080p_i_and_p_pair(lib):
    """one full-size IDR + P pair with the session's defaults (tiles in the IDR picture, pre-search): about 10 s of numpy"""
    w, h, n = 1920, 1080, 2
    cfg = small_cfg(w, h, 8, qp=30, keyint=8, level_idc=120, me_range=16, pre_search=1)
    frames = [util.synth_frame(h, w, seed=47, shift=(5 * i, 2 * i)) for i in range(n)]
    stream, recs = session(cfg, frames)
    st = S.parse_stream(stream)
    assert [p.slices[0]["slice_type"] for p in st.pictures] == [2, 1] and (st.pictures[0].w, st.pictures[0].h) == (1920, 1080)
    check_recon(st, recs)
