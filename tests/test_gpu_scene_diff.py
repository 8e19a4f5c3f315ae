"""GPU: `k_scene_diff`, the scene-cut detector every session runs by default (mihevc_config.scenecut), through mihevc_k_scene_diff (the session's launcher on
zeroed sums) against tests/scene_ref.py, exactly: shapes from 4 sampled positions to a row longer than a workgroup's stride, two sizes that are no multiple of 4, one 1920x1080 pair at which a lane
takes more than one turn of the grid-stride loop, 8 and 10 bit, 2 / 3 / 7 pictures, a pitch of its own for every picture with garbage beyond the width, the
largest sum and the sum 0.  Then one session over two chunks: its IDR pictures are those of the planner (the Python statement of tests/test_gop_plan_cpu.py)
fed with the reference's sums."""
import numpy as np
import pytest

from tests import scene_ref as S
from tests import util
from tests.test_gop_plan_cpu import MAX_LANES, chunks_of, reference_plan, stream_gops

pytestmark = pytest.mark.gpu

# the last two: sizes that are no multiple of 4, where ceil(w / 4) columns and ceil(h / 4) rows are sampled and not w / 4, h / 4 (a session never has such a
# size; the entry takes it, and on every other shape a kernel that rounds down would pass)
SHAPES = ((8, 8), (64, 64), (136, 72), (72, 104), (1928, 24), (70, 38), (13, 9))


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    lib = _lib.load()
    assert lib.mihevc_device_count() >= 1
    return lib


def pictures(rng, n, w, h, bd, kind):
    """n planes, each with a pitch of its own (w + 0 .. 37) and random samples beyond the width"""
    dt, top = (np.uint8, 255) if bd == 8 else (np.uint16, 1023)
    out = []
    for i in range(n):
        p = rng.integers(0, top + 1, (h, w + int(rng.integers(0, 38))), dtype=dt)
        if kind == "extremes":
            p[:, :w] = top if i & 1 else 0
        elif kind == "identical" and i:
            p[:, :w] = out[0][:, :w]
        out.append(p)
    return out


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("w,h", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_sums_equal_the_reference(lib, w, h, bd):
    rng = np.random.default_rng(w * 131 + h * 7 + bd)
    top = 255 if bd == 8 else 1023
    for n in (2, 3, 7):
        for kind in ("random", "extremes", "identical"):
            planes = pictures(rng, n, w, h, bd, kind)
            assert len({p.shape[1] for p in planes}) > 1 or n == 2
            rc, got = util.scene_diff(lib, planes, w, h, bd)
            want = S.scene_sums(planes, w, h)
            assert rc == 0 and got == want, (n, kind, got, want)
            if kind == "extremes":
                assert want[1:] == [top * S.sampled_positions(w, h)] * (n - 1)
            if kind == "identical":
                assert want == [0] * n


def test_one_picture_gives_zero(lib):
    assert util.scene_diff(lib, [np.full((8, 8), 7, np.uint8)], 8, 8, 8) == (0, [0])


@pytest.mark.parametrize("bd", [8, 10])
def test_a_1080p_pair_takes_more_than_one_turn_of_the_loop(lib, bd):
    """129,600 sampled positions against 32 x 256 = 8,192 lanes"""
    w, h = 1920, 1080
    assert S.sampled_positions(w, h) > 32 * 256
    rng = np.random.default_rng(bd)
    for kind in ("random", "extremes"):
        planes = pictures(rng, 2, w, h, bd, kind)
        rc, got = util.scene_diff(lib, planes, w, h, bd)
        assert rc == 0 and got == S.scene_sums(planes, w, h), kind


def planned(frames, w, h, keyint, min_keyint, lanes, carry=True, leftover=False):
    """the IDR pictures of the planner as tests/test_gop_plan_cpu.py restates it, chunk by chunk, fed with the reference's sums.  carry = False: a planner that forgets its
    running mean between chunks; leftover = True: sums that are not zeroed, so a chunk's are added to the chunk's before it"""
    out, state, before = [], {"scene_avg": 0.0}, None
    for pos, m, flushing in chunks_of(len(frames), keyint, lanes):
        diff = S.scene_sums([f.y for f in frames[pos:pos + m]], w, h)
        if leftover and before is not None:
            diff = [a + b for a, b in zip(diff, before)]
        before = diff
        if not carry:
            state = {"scene_avg": 0.0}
        starts = reference_plan(diff, float(S.sampled_positions(w, h)), m, keyint, min_keyint, True, flushing, MAX_LANES, state)
        out += [pos + a for a, _ in stream_gops(starts, m, keyint, True)]
    return out


def test_a_session_cuts_where_the_planner_fed_with_the_reference_sums_does(lib):
    """24 pictures of 64x64, keyint 6, two GOPs in flight: two chunks of 12.  A scene change at picture 5; pictures 13 .. 19 each show a new scene (a run of jumps, cut at its
    last picture), the rest moves calmly (about 10 grey levels a picture against 23 .. 30).  The second chunk's jumps are jumps only against the running mean of the FIRST chunk:
    its own median is one of them, so a planner that starts afresh takes picture 13 for ordinary and cuts nowhere; and sums left over from the first chunk would move the cuts
    too.  Both are asserted on the reference side, so the clip cannot quietly stop binding."""
    from hevc_amd import _lib
    from hevc_amd.encoder import Encoder
    w, h, n, keyint, min_keyint, lanes = 64, 64, 24, 6, 1, 2
    frames = [util.synth_frame(h, w, seed=40 + (0 if i < 5 else 1 if i < 13 else min(i, 19) - 11), shift=(i, i // 2)) for i in range(n)]
    cfg = _lib.default_config()
    cfg.width, cfg.height, cfg.keyint, cfg.min_keyint, cfg.me_range, cfg.gops_in_flight, cfg.qp = w, h, keyint, min_keyint, 8, lanes, 30
    assert cfg.scenecut == 1 and cfg.gop_balance == 1
    with Encoder(cfg, device=0) as enc:
        for f in frames:
            enc.send(*util.planes(f, 8))
        enc.flush()
        for _ in enc.packets():
            pass
        got = [i for i in range(n) if enc.frame_info(i)[1] == 2]
    assert [(p, m) for p, m, _ in chunks_of(n, keyint, lanes)] == [(0, 12), (12, 12)]
    want = planned(frames, w, h, keyint, min_keyint, lanes)
    assert want == [0, 5, 9, 12, 16, 19]
    assert planned(frames, w, h, keyint, min_keyint, lanes, carry=False) != want and planned(frames, w, h, keyint, min_keyint, lanes, leftover=True) != want
    assert got == want, (got, want)
