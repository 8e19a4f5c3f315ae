"""CPU: the GOP planner of hevc_amd/csrc/gop_plan.h, run on arrays through tests/emu/gop_plan.cpp.  Without cuts against util.idr_positions; the lane order
against its definition; with cuts against `reference_plan` below, a second statement of the rules that shares no code and no structure with the header
(classify every picture first, then the candidates, then the min-keyint and lane conditions on explicit GOP lengths).  No expected value comes from the
function under test."""
import ctypes as C

import numpy as np
import pytest

from tests import util

MAX_LANES = 16          # csrc/device.h
CUT_ABS, CUT_RATIO = 8.0, 1.8


class Planner:
    """a session's planner: one call per chunk, the state carried along"""

    def __init__(self, lib=None):
        self.lib = lib or util.stepped_library()
        self.scene_avg, self.last_gop_len = C.c_double(0), C.c_int(0)

    def chunk(self, n, keyint, min_keyint=0, balance=True, flushing=False, diff=None, per=1.0, max_lanes=MAX_LANES):
        d = np.ascontiguousarray(diff if diff is not None else [], dtype=np.uint64)
        gstart, glen, prev, batch = (np.full(n, -1, np.int32) for _ in range(4))
        steps = C.c_int(0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        gops = self.lib.emu_gop_plan(p(d), C.c_int(len(d)), C.c_double(per), n, keyint, min_keyint, int(balance), int(flushing), max_lanes,
                                     C.byref(self.scene_avg), C.byref(self.last_gop_len), p(gstart), p(glen), p(prev), p(batch), C.byref(steps))
        assert gops >= 1
        return {"gstart": gstart[:gops].tolist(), "glen": glen[:gops].tolist(), "prev_len": prev[:gops].tolist(), "batch": batch[:steps.value].tolist()}


def chunks_of(n, keyint, lanes):
    """(first picture, pictures, flushing) of the chunks a session cuts n pictures into: lanes x keyint at a time, the rest at the flush"""
    out, pos = [], 0
    while pos < n:
        m = min(lanes * keyint, n - pos)
        out.append((pos, m, m < lanes * keyint))
        pos += m
    return out


def gop_lengths(length, keyint, balance):
    """the fewest GOPs keyint allows for `length` pictures: near-equal, or keyint long with the remainder last"""
    g = -(-length // keyint)
    if balance:
        return [length // g + (j < length % g) for j in range(g)]
    return [keyint] * (length // keyint) + ([length % keyint] if length % keyint else [])


def reference_plan(diff, per, n, keyint, min_keyint, balance, flushing, max_lanes, state):
    """Segment starts of one chunk, from the rules as DESIGN.md and the header's comment state them.  state: {'scene_avg': float}, updated."""
    d = [float(x) / per for x in diff]
    avg = state["scene_avg"]
    stand_in = sorted(int(x) for x in diff[1:])[(n - 1) // 2] / per if avg <= 0 else None      # the median, while the mean has seen no ordinary picture
    # 1. every picture is a jump or ordinary; only ordinary pictures move the mean
    jump = [False] * n
    for i in range(1, n):
        base = avg if avg > 0 else stand_in
        jump[i] = d[i] > CUT_ABS and d[i] > CUT_RATIO * base
        if not jump[i]:
            avg = 0.8 * avg + 0.2 * d[i] if avg > 0 else d[i]
    state["scene_avg"] = avg
    # 2. a run of jumps offers its last picture
    candidates = [i for i in range(1, n) if jump[i] and not (i + 1 < n and jump[i + 1])]
    # 3. a candidate is taken when every GOP of the segment it closes and the chunk's tail keep min-keyint pictures, and the lanes suffice
    floor = max(1, min_keyint)
    starts, closed = [0], 0
    for i in candidates:
        lens = gop_lengths(i - starts[-1], keyint, balance)
        if min(lens) < floor or (not flushing and n - i < floor):
            continue
        if closed + len(lens) + len(gop_lengths(n - i, keyint, False)) > max_lanes:
            continue
        closed += len(lens)
        starts.append(i)
    return starts


def stream_gops(starts, n, keyint, balance):
    """[(first picture, length)] of the chunk's GOPs in stream order"""
    out = []
    for a, b in zip(starts, starts[1:] + [n]):
        at = a
        for ln in gop_lengths(b - a, keyint, balance):
            out.append((at, ln))
            at += ln
    return out


def expected_lanes(gops, last_gop_len):
    """the lanes of a chunk from its GOPs in stream order: longest first, equal lengths in stream order"""
    order = sorted(range(len(gops)), key=lambda k: -gops[k][1])
    glen = [gops[k][1] for k in order]
    return {"gstart": [gops[k][0] for k in order], "glen": glen, "prev_len": [gops[k - 1][1] if k else last_gop_len for k in order],
            "batch": [sum(1 for ln in glen if ln > t) for t in range(glen[0])]}


# ---- (a) no cuts: the IDR places of util.idr_positions -------------------------------------------------------------------------------------------
GRID = [(n, keyint, lanes, balance) for n in (1, 2, 29, 89, 90, 91, 300, 301, 359, 360, 361, 725) for keyint, lanes in ((90, 4), (30, 4), (90, 1), (48, 3), (7, 16), (240, 2))
        for balance in (True, False)]


@pytest.mark.parametrize("detector", [False, True])
def test_no_cuts_matches_idr_positions(detector):
    assert (300, 90, 4, True) in GRID
    assert util.idr_positions(300, 90, 4, True) == [0, 75, 150, 225]
    for n, keyint, lanes, balance in GRID:
        pl, got = Planner(), []
        for pos, m, flushing in chunks_of(n, keyint, lanes):
            # detector on: a calm clip (every difference 3 grey levels) has no cut either
            diff = np.full(m, 3, np.uint64) if detector and m > 1 else None
            r = pl.chunk(m, keyint, min_keyint=1, balance=balance, flushing=flushing, diff=diff)
            got += [pos + g for g in r["gstart"]]
        assert sorted(got) == util.idr_positions(n, keyint, lanes, balance), (n, keyint, lanes, balance)


# ---- (b) lane order, batch, prev_len across chunks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,keyint,lanes,balance", [(560, 90, 4, False), (560, 90, 4, True), (301, 90, 4, True), (725, 48, 3, False), (100, 7, 16, True), (200, 90, 4, False)])
def test_lane_order_batch_and_prev_len(n, keyint, lanes, balance):
    idr = util.idr_positions(n, keyint, lanes, balance)
    lengths = {a: b - a for a, b in zip(idr, idr[1:] + [n])}          # stream GOP lengths by first picture
    pl, last = Planner(), 0
    cks = chunks_of(n, keyint, lanes)
    assert len(cks) >= 2 or n < lanes * keyint
    for pos, m, flushing in cks:
        gops = [(a - pos, lengths[a]) for a in idr if pos <= a < pos + m]
        want = expected_lanes(gops, last)
        got = pl.chunk(m, keyint, balance=balance, flushing=flushing)
        assert got == want, (pos, m)
        assert got["glen"] == sorted(got["glen"], reverse=True) and len(got["batch"]) == got["glen"][0]
        assert all(got["batch"][t] == sum(1 for ln in got["glen"] if ln > t) for t in range(len(got["batch"])))
        last = gops[-1][1]
        assert pl.last_gop_len.value == last


# ---- (c) cuts -------------------------------------------------------------------------------------------------------------------------------------------
def calm(n, jumps, level=2, high=40, per=1):
    d = np.full(n, level * per, np.uint64)
    d[0] = 0
    for i in jumps:
        d[i] = high * per
    return d


def check_against_reference(diff, n, keyint, min_keyint, balance, flushing, per=1.0, scene_avg=0.0, last_gop_len=0, max_lanes=MAX_LANES, lib=None):
    state = {"scene_avg": scene_avg}
    starts = reference_plan(diff, per, n, keyint, min_keyint, balance, flushing, max_lanes, state)
    want = expected_lanes(stream_gops(starts, n, keyint, balance), last_gop_len)
    pl = Planner(lib)
    pl.scene_avg.value, pl.last_gop_len.value = scene_avg, last_gop_len
    got = pl.chunk(n, keyint, min_keyint=min_keyint, balance=balance, flushing=flushing, diff=diff, per=per, max_lanes=max_lanes)
    assert got == want, (starts, got)
    assert pl.scene_avg.value == state["scene_avg"]          # the same operations in the same order: it feeds the next chunk
    assert len(got["glen"]) <= max_lanes and sum(got["glen"]) == n
    return starts


@pytest.mark.parametrize("balance", [True, False])
def test_single_jump(balance):
    starts = check_against_reference(calm(200, [100]), 200, 90, 10, balance, False)
    assert starts == [0, 100]          # (the reference itself, on a case that can be read off)
    assert stream_gops(starts, 200, 90, True) == [(0, 50), (50, 50), (100, 50), (150, 50)]


@pytest.mark.parametrize("balance", [True, False])
def test_run_of_jumps_is_cut_at_its_last_picture(balance):
    assert check_against_reference(calm(200, [100, 101, 102]), 200, 90, 10, balance, False) == [0, 102]
    assert check_against_reference(calm(200, [60, 61, 140]), 200, 90, 10, balance, True) == [0, 61, 140]


@pytest.mark.parametrize("balance", [True, False])
def test_min_keyint_at_both_ends(balance):
    assert check_against_reference(calm(200, [5]), 200, 90, 10, balance, False) == [0]              # the GOP it closes would have 5 pictures
    assert check_against_reference(calm(200, [10]), 200, 90, 10, balance, False) == [0, 10]
    assert check_against_reference(calm(200, [195]), 200, 90, 10, balance, False) == [0]            # the GOP it opens would, and another chunk follows
    assert check_against_reference(calm(200, [195]), 200, 90, 10, balance, True) == [0, 195]        # the stream's last chunk may end short
    assert check_against_reference(calm(200, [190]), 200, 90, 10, balance, False) == [0, 190]
    # a segment of 95 pictures is two GOPs: balanced 48 + 47, keyint-spaced 90 + 5
    assert check_against_reference(calm(200, [95]), 200, 90, 10, balance, False) == ([0, 95] if balance else [0])


@pytest.mark.parametrize("min_keyint,want", [(1, [0, 1, 100]), (10, [0, 100])])
def test_jump_at_the_sessions_second_picture(min_keyint, want):
    # no mean yet: the chunk's median (2) stands in, the jump is seen, and it never becomes the mean the later jump is measured against
    for per in (1, 1 << 12):
        diff = calm(200, [1, 100], per=per)
        assert check_against_reference(diff, 200, 90, min_keyint, True, False, per=float(per)) == want
    # with a mean from earlier chunks the same picture is measured against it
    assert check_against_reference(calm(200, [1, 100]), 200, 90, 1, True, False, scene_avg=30.0, last_gop_len=75) == [0, 100]
    assert check_against_reference(calm(200, [1, 100]), 200, 90, 1, True, False, scene_avg=3.0, last_gop_len=75) == [0, 1, 100]


@pytest.mark.parametrize("balance", [True, False])
def test_more_cuts_than_lanes(balance):
    jumps = list(range(8, 200, 8))          # 24 candidates
    starts = check_against_reference(calm(200, jumps), 200, 90, 1, balance, False)
    assert starts == [0] + jumps[:15]       # 15 segments of one GOP each closed, and the 80 pictures behind the 15th cut are the 16th lane
    assert len(check_against_reference(calm(200, jumps), 200, 90, 1, balance, False, max_lanes=4)) == 4


def test_random_clips_against_the_reference():
    rng = np.random.default_rng(7)
    for _ in range(300):
        n = int(rng.integers(2, 400))
        keyint = int(rng.integers(max(1, (n + MAX_LANES - 1) // MAX_LANES), 241))
        min_keyint = int(rng.integers(0, keyint))
        per = float(rng.choice([1, 3, 480 * 270, 480 * 270 * 4]))
        d = rng.integers(0, 6, n).astype(np.float64)
        high = rng.random(n) < 0.06
        d[high] += rng.integers(5, 60, int(high.sum()))
        diff = np.floor(d * per).astype(np.uint64)
        check_against_reference(diff, n, keyint, min_keyint, bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), per=per,
                                scene_avg=float(rng.choice([0.0, 1.5, 4.0])), last_gop_len=int(rng.integers(0, 91)))
