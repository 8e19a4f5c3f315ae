"""CPU: the rate controller of hevc_amd/csrc/ratectl.h, run on arrays through tests/emu/ratectl.cpp, against the independent statement
tests/ratectl_ref.py and against the properties §5b promises.  Pure host code with deterministic inputs: QPs in, QPs out.

Comparison rules: QPs exactly, learned state to 1e-12 relative (sums of under 200 float64 terms: four orders above rounding).  The model reports for every
decision its distance to the nearest threshold; a decision closer than 1e-9 is undecidable (exp2 / log2 may differ in the last place between libm and Python)
and would be left out.  Every test below uses fixed seeds for which the model reports ZERO such decisions, and asserts that: change a seed, not the epsilon.

p_slots (a P step's CABAC size is known p_slots steps later): a session passes ring - 1, and hevc_amd/csrc/session.cpp opens with a ring of 8 slots below level 5
and of kRing = 12 (hevc_amd/csrc/session.h) from level 5 on: 7 and 11.  1, 2 and 5 are not in use; they put the size lag in front of, at and just behind the
estimate lag of two steps, where the two visibility rules cross."""
import ctypes as C
import functools
import math
import random

import pytest

from tests import ratectl_ref as R
from tests import util

P_SLOTS = (1, 2, 5, 7, 11)
REL = 1e-12


class Header:
    """hevc_amd/csrc/ratectl.h behind the C ABI of tests/emu/ratectl.cpp, with the method names of ratectl_ref.Model"""
    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            L = util.stepped_library()
            L.emu_rc_create.restype = C.c_void_p
            L.emu_rc_create.argtypes = [C.c_int] * 8 + [C.c_double, C.c_int]
            L.emu_rc_destroy.argtypes = [C.c_void_p]
            L.emu_rc_begin_chunk.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
            L.emu_rc_step_qp.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
            L.emu_rc_want_idr.argtypes = [C.c_void_p, C.c_int, C.c_ulonglong, C.c_int]
            L.emu_rc_measure_rho.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
            L.emu_rc_idr_settled.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
            L.emu_rc_learn.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
            L.emu_rc_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            L.emu_rc_set_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            L.emu_rc_gop_step.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
            cls._lib = L
        return cls._lib

    def __init__(self, *args):
        self.L = self.lib()
        self.h = self.L.emu_rc_create(*args)
        self.qp_i, self.qp_p = args[6], args[7]

    def __del__(self):
        self.L.emu_rc_destroy(self.h)

    @staticmethod
    def _arrays(recs):
        n = len(recs)
        return ((C.c_int * n)(*[r.qp for r in recs]), (C.c_int * n)(*[r.type for r in recs]), (C.c_longlong * n)(*[r.bits for r in recs]),
                (C.c_ulonglong * n)(*[r.est for r in recs]), (C.c_int * n)(*[int(r.est_known) for r in recs]))

    def begin_chunk(self, bf, glen):
        self.L.emu_rc_begin_chunk(self.h, int(bf), (C.c_int * len(glen))(*glen), len(glen))

    def step_qp(self, g, t, recs):
        return self.L.emu_rc_step_qp(self.h, g, t, len(recs), *self._arrays(recs))

    def want_idr(self, g, est, qa):
        return self.L.emu_rc_want_idr(self.h, g, est, qa)

    def trial_qp(self, want):
        return self.L.emu_rc_trial_qp(want)

    def redo_idr(self, want, qa):
        return bool(self.L.emu_rc_redo_idr(want, qa))

    def measure_rho(self, est_p, qp_trial, est_i, qa):
        n = len(est_p)
        self.L.emu_rc_measure_rho(self.h, n, (C.c_ulonglong * n)(*est_p), (C.c_int * n)(*qp_trial), (C.c_ulonglong * n)(*est_i), (C.c_int * n)(*qa))

    def idr_settled(self, qps):
        self.L.emu_rc_idr_settled(self.h, (C.c_int * len(qps))(*qps), len(qps))

    def learn(self, lanes):
        off = [0]
        for recs in lanes:
            off.append(off[-1] + len(recs))
        self.L.emu_rc_learn(self.h, len(lanes), (C.c_int * len(off))(*off), *self._arrays([r for recs in lanes for r in recs]))

    def _raw(self):
        d, i = (C.c_double * 4)(), (C.c_int * 4)()
        self.L.emu_rc_get_state(self.h, d, i)
        return list(d), list(i)

    def get_state(self):
        d, i = self._raw()
        return dict(ratio_i=d[0], ratio_p=d[1], rho_pi=d[2], beta_bp=d[3], idr_qp_hint=i[0], rho_measured=bool(i[1]))

    def set_state(self, **kw):
        s = self.get_state()
        s.update(kw)
        self.L.emu_rc_set_state(self.h, (C.c_double * 4)(s["ratio_i"], s["ratio_p"], s["rho_pi"], s["beta_bp"]), (C.c_int * 2)(s["idr_qp_hint"], int(s["rho_measured"])))

    @property
    def rho_measured(self):
        return self.get_state()["rho_measured"]

    @property
    def b_offset(self):
        return self._raw()[1][3]


def gop_step(bf, t, n):
    out = (C.c_int * 6)()
    Header.lib().emu_rc_gop_step(int(bf), t, n, out)
    return list(out)      # pos, type, cur, prev, nxt, ref_pos


def both(crf=19, maxrate=1000, bufsize=1200, fps=(30, 1), b_off=-1, share=1.0, p_slots=7, qp_cfg=-1):
    args = (qp_cfg, maxrate, bufsize, fps[0], fps[1], b_off, crf - 1, crf + 2, share, p_slots)
    return Header(*args), R.Model(*args)


def same_state(h, m, what=""):
    hs, ms = h.get_state(), m.get_state()
    for k in ("ratio_i", "ratio_p", "rho_pi", "beta_bp"):
        assert math.isfinite(hs[k]) and abs(hs[k] - ms[k]) <= REL * abs(ms[k]), (what, k, hs[k], ms[k])
    assert (hs["idr_qp_hint"], hs["rho_measured"]) == (ms["idr_qp_hint"], ms["rho_measured"]), (what, hs, ms)


def random_state(rng):
    """learned state anywhere within its clamps (the ratios have none: what estimates are off by, and well beyond)"""
    return dict(ratio_i=rng.uniform(0.5, 2.0), ratio_p=rng.uniform(0.5, 2.0), rho_pi=2.0 ** rng.uniform(-8, 0), beta_bp=rng.uniform(0.05, 1.5))


# ================================================================ a. GOP structure
@pytest.mark.parametrize("bf", [0, 1])
def test_gop_structure_keeps_every_reference_alive(bf):
    """three reconstruction buffers simulated through gop_step for every GOP length 1..40: what a step reads is still there, what it writes nobody needs"""
    for n in range(1, 41):
        steps = [gop_step(bf, t, n) for t in range(n)]
        want = R.gop_table(bf, n)
        assert sorted(s[0] for s in steps) == list(range(n)), (n, "positions are no permutation")
        types = {s[0]: s[1] for s in steps}
        assert [types[p] for p in range(n)] == R.display_types(bf, n), n
        assert types[0] == R.I and steps[0][0] == 0 and types[n - 1] != R.B
        for p in range(n):
            if types[p] == R.B:
                assert 0 < p < n - 1 and types[p - 1] != R.B and types[p + 1] != R.B, (n, p)
        assert bf or all(s[0] == t for t, s in enumerate(steps))
        holds = {}
        for t, (pos, typ, cur, prev, nxt, ref_pos) in enumerate(steps):
            assert (pos, typ) == (want[t].pos, want[t].type), (n, t)
            reads = [] if typ == R.I else [prev] if typ == R.P else [prev, nxt]
            assert cur in (0, 1, 2) and cur not in reads, (n, t, "writes a buffer it reads")
            if typ != R.I:
                assert ref_pos == want[t].refs[0] and holds.get(prev) == ref_pos, (n, t, "list 0", holds, steps[t])
            if typ == R.B:
                assert (ref_pos, holds.get(nxt)) == (pos - 1, pos + 1) and want[t].refs == (pos - 1, pos + 1), (n, t, "list 1", holds, steps[t])
            # what later steps still read must not sit in the buffer this step overwrites
            if cur in holds:
                for u in range(t, n):
                    assert holds[cur] not in want[u].refs, (n, t, u, "overwrites a picture step %d predicts from" % u)
            holds[cur] = pos


# ================================================================ b. want_idr
def modelled_idr(est, ratio_i, qa, q):
    return max(1.0, est / 16.0 * ratio_i) * 2.0 ** ((qa - q) / 6.0)


def test_want_idr_against_the_model_and_its_own_promises():
    rng = random.Random(11)
    ests = [int(16 * 10 ** (k + rng.random())) for k in range(1, 8)]       # 1/16 bit: ten bits to a hundred million, one per decade
    calls = undecidable = 0
    for n in (1, 2, 3, 30, 90):
        for bf in (0, 1):
            for bufsize_on in (0, 1):
                for share in (1.0, 0.125):
                    for fps in ((30, 1), (30000, 1001)):
                        crf, st = rng.choice((10, 19, 28)), random_state(rng)
                        rates = sorted(rng.sample((150, 400, 1000, 2500, 6000, 15000, 40000), 3))
                        buf = int(1.2 * rates[1]) * bufsize_on
                        pair = [both(crf, r, buf, fps, share=share) for r in rates]
                        for h, m in pair:
                            h.set_state(**st); m.set_state(**st)
                            h.begin_chunk(bf, [90, n]); m.begin_chunk(bf, [90, n])
                        qp_i = crf - 1
                        for qa in range(52):
                            last = [0, 0, 0]
                            for est in ests:
                                got = [h.want_idr(1, est, qa) for h, _ in pair]
                                for k, (h, m) in enumerate(pair):
                                    before = m.undecidable
                                    want = m.want_idr(1, est, qa)
                                    calls += 1
                                    if m.undecidable > before:
                                        undecidable += 1
                                        continue
                                    assert got[k] == want, (n, bf, buf, share, fps, rates[k], qa, est, st, got[k], want)
                                    assert qp_i <= got[k] <= 51
                                    size = modelled_idr(est, st["ratio_i"], qa, got[k])
                                    cap = 0.85 * 0.9 * share * buf * 1000.0 if buf else math.inf
                                    assert got[k] == 51 or size <= cap * (1 + REL), (size, cap)
                                    assert got[k] >= last[k], ("finer for a larger estimate", n, bf, rates[k], qa, est)
                                    if n == 1:        # an IDR-only GOP: the finest QP whose picture fits budget and cap, else 51
                                        room = min(cap, 0.985 * share * rates[k] * 1000.0 * fps[1] / fps[0])
                                        if size <= room * (1 + REL):
                                            assert got[k] == qp_i or modelled_idr(est, st["ratio_i"], qa, got[k] - 1) > room * (1 - REL)
                                        else:
                                            assert got[k] == 51
                                assert got[0] >= got[1] >= got[2], ("coarser under a higher cap", n, bf, rates, qa, est, got)
                                last = got
    assert undecidable == 0 and calls > 20000, (undecidable, calls)


# ================================================================ c. step_qp / decide_p
def visible(recs, t, p_slots, garbage=None):
    """lane records as a session holds them in front of step t: the CABAC size of step j only once its ring slot has been handed out again (j <= t - p_slots; the
    job that delivers it delivers the estimate too), the estimate with a lag of two steps; the IDR picture's estimate from step 0.  garbage: a random.Random that
    fills every field the controller may not read"""
    out = []
    for j, r in enumerate(recs[:t]):
        sized = 1 <= j <= t - p_slots
        known = j == 0 or j <= t - 2 or sized
        bits, est, ek = (r.bits if sized else -1), (r.est if known else 0), (r.est_known and known)
        if garbage is not None:
            if not sized:
                bits = garbage.choice((0, 1, 10 ** 9, garbage.randrange(1, 10 ** 7)))
            if not known:
                est, ek = garbage.randrange(0, 10 ** 9), False
            elif j > t - 2 and j != 0:      # sized, but outside the estimate lag: the flag is not read there
                ek = garbage.random() < 0.5
        out.append(R.Rec(r.qp, r.type, bits, est, ek))
    return out


def random_gop(rng, h, m, shadow, n, bf, p_slots, garbage, checks):
    """one lane through a GOP of n pictures on random sizes.  Header and model side by side; `shadow` is a second header that sees garbage wherever the session
    shows nothing.  Returns the number of P decisions compared."""
    types, kqpb = R.step_types(bf, n), h.b_offset
    for rc in (h, m, shadow):
        rc.begin_chunk(bf, [n])
    qa = h.step_qp(0, 0, [])
    assert qa == m.step_qp(0, 0, []) == shadow.step_qp(0, 0, [])
    q0 = rng.randrange(h.qp_i, 52)
    for rc in (h, m, shadow):
        rc.idr_settled([q0])
    # content sized to the cap: its P pictures would spend the GOP's delivery at some QP between the CRF's and 51 (c: IDR bits at QP 0), and it
    # gets harder or easier at one picture of the GOP, so that the walk has somewhere to go
    rho = 2.0 ** rng.uniform(-6, -1)
    c = m.budget[0] / n / rho * 2 ** (rng.uniform(h.qp_p - 4, 55) / 6)
    jump_at, jump = rng.randrange(1, n + 1), 2.0 ** rng.uniform(-2, 2)
    recs = [R.Rec(q0, R.I, int(c * 2 ** (-q0 / 6)), int(16 * c * 2 ** (-q0 / 6) * rng.uniform(0.8, 1.2)), True)]
    anchor, compared = q0, 0
    for t in range(1, n):
        view = visible(recs, t, p_slots)
        if types[t] == R.B:
            qp = h.step_qp(0, t, [])
            assert qp == m.step_qp(0, t, []) == shadow.step_qp(0, t, []) == min(51, anchor + kqpb), (t, qp, anchor, kqpb)
        else:
            before = m.undecidable
            qp, want = h.step_qp(0, t, view), m.step_qp(0, t, view)
            assert m.undecidable == before, ("undecidable: change the seed", m.decisions[-1])
            assert qp == want, (n, bf, p_slots, t, qp, want, m.decisions[-1], view)
            assert qp == shadow.step_qp(0, t, visible(recs, t, p_slots, garbage)), (n, bf, p_slots, t, "reads a field the session has not filled")
            assert h.qp_p <= qp <= 51
            if t == 1:
                assert qp >= q0, "first P picture finer than its IDR"
            else:
                assert qp - anchor in (-1, 0, 1, 2, 3), (t, qp, anchor)
                checks[qp - anchor] = checks.get(qp - anchor, 0) + 1
            anchor, compared = qp, compared + 1
        # the plant: the controller's own rate law with a lot of noise; now and then a picture the session has nothing for
        w = (rho if types[t] == R.P else rho * 0.4 * 2 ** (kqpb / 6)) * (jump if t >= jump_at else 1.0)
        bits = int(c * w * 2 ** (-qp / 6) * math.exp(rng.gauss(0, 0.35)))
        est = int(16 * bits * rng.uniform(0.75, 1.2))
        if rng.random() < 0.08:
            bits, est = -1, 0
        elif rng.random() < 0.03:
            est = 0
        recs.append(R.Rec(qp, types[t], bits, est, rng.random() < 0.97))
    return compared


@pytest.mark.parametrize("bf", [0, 1])
@pytest.mark.parametrize("p_slots", P_SLOTS)
def test_step_qp_against_the_model_over_random_lane_histories(bf, p_slots):
    rng, garbage = random.Random(100 * p_slots + bf), random.Random(7)
    compared, moves = 0, {}
    for trial in range(36):
        n = (2, 3, 4, 5, 90, 89)[trial] if trial < 6 else rng.randrange(2, 91)
        crf = rng.choice((12, 19, 27))
        # caps from hopeless to generous: the walk must show every move, the floor at the CRF's QP and the ceiling at 51
        maxrate = rng.choice((60, 250, 1000, 4000, 16000))
        args = dict(crf=crf, maxrate=maxrate, bufsize=int(1.2 * maxrate), b_off=rng.choice((-1, 0, 2, 4)), p_slots=p_slots)
        (h, m), (shadow, _) = both(**args), both(**args)
        st = random_state(rng)
        for rc in (h, m, shadow):
            rc.set_state(**st)
        compared += random_gop(rng, h, m, shadow, n, bf, p_slots, garbage, moves)
        assert m.undecidable == 0
    assert compared > 500 and all(moves.get(k, 0) > 0 for k in (-1, 0, 1, 2, 3)), (compared, moves)       # every move of the walk was taken


@pytest.mark.parametrize("b_off,want", [(-1, 2), (0, 0), (1, 1), (2, 2), (7, 7), (8, 8), (9, 8), (30, 8)])
def test_b_qp_offset_is_clamped_at_eight(b_off, want):
    h, m = both(b_off=b_off)
    assert h.b_offset == m.b_offset == want
    for rc in (h, m):
        rc.begin_chunk(1, [5])
        rc.step_qp(0, 0, [])
        rc.idr_settled([47])
    assert h.step_qp(0, 1, [R.Rec(47, R.I, -1, 16 * 50000, True)]) == m.step_qp(0, 1, [R.Rec(47, R.I, -1, 16 * 50000, True)])
    anchor = m.anchor_qp[0]
    assert h.step_qp(0, 2, []) == m.step_qp(0, 2, []) == min(51, anchor + want)


def test_without_a_cap_or_with_a_fixed_qp_the_controller_stays_out():
    for kw in (dict(maxrate=0), dict(qp_cfg=30)):
        h, m = both(**kw)
        for rc in (h, m):
            rc.begin_chunk(1, [6])
        assert [h.step_qp(0, t, []) for t in range(6)] == [m.step_qp(0, t, []) for t in range(6)] == [18, 21, 23, 21, 23, 21]


# ================================================================ d. measure_rho, learn, idr_settled
def random_chunk(rng, bf, lanes, kqpb, scale_p=1.0, scale_b=1.0):
    """finished records of a chunk: sizes around the rate law, some pictures without a size, without an estimate, of size 0"""
    glen = [rng.randrange(1, 31) for _ in range(lanes)]
    out = []
    for n in glen:
        types, q0, c = R.step_types(bf, n), rng.randrange(15, 45), 10.0 ** rng.uniform(5, 7)
        recs = []
        for t in range(n):
            qp = q0 if t == 0 else min(51, q0 + rng.randrange(0, 8))
            w = 1.0 if t == 0 else 0.1 * scale_p if types[t] == R.P else 0.04 * scale_p * scale_b * 2 ** (kqpb / 6)
            bits = int(c * w * 2 ** (-qp / 6) * rng.uniform(0.7, 1.4))
            est = int(16 * bits * rng.uniform(0.7, 1.14))
            u = rng.random() if t else 0.5 + rng.random() / 2 if rng.random() < 0.9 else 0.0      # an IDR picture is never empty, but its size may be missing
            if u < 0.06:
                bits = -1
            elif u < 0.10:
                bits = 0
            elif u < 0.15:
                est = 0
            recs.append(R.Rec(qp, types[t], bits, est, True))
        out.append(recs)
    return glen, out


@pytest.mark.parametrize("bf", [0, 1])
def test_learn_against_the_model_over_chunks_in_sequence(bf):
    rng = random.Random(5 + bf)
    h, m = both(b_off=3)
    hit = set()
    # the scales push P / I and B / P far out of range and back, so that both clamps are reached from inside and left again
    for chunk, (sp, sb) in enumerate([(1, 1), (1, 1), (40, 1), (40, 60), (40, 60), (1, 1)] + [(1e-2, 1)] * 10 + [(1, 0.05)] * 8 + [(1, 1), (1, 1)]):
        glen, lanes = random_chunk(rng, bf, rng.randrange(1, 7), 3, sp, sb)
        for rc in (h, m):
            rc.begin_chunk(bf, glen)
            rc.learn(lanes)
        same_state(h, m, chunk)
        s = h.get_state()
        assert 1 / 256 <= s["rho_pi"] <= 1.0 and 0.05 <= s["beta_bp"] <= 1.5
        hit |= {(k, s[k]) for k in ("rho_pi", "beta_bp") if s[k] in (1 / 256, 1.0, 0.05, 1.5)}
    assert {("rho_pi", 1.0), ("rho_pi", 1 / 256)} <= hit and (not bf or {("beta_bp", 1.5), ("beta_bp", 0.05)} <= hit), hit
    s = h.get_state()
    assert 1 / 256 < s["rho_pi"] < 1.0 and 0.05 < s["beta_bp"] < 1.5            # ... and left again
    assert bf or s["beta_bp"] == 0.45                                        # no B picture, nothing learned about them


def test_learn_halves_towards_the_chunk_and_skips_lanes_without_an_idr_size():
    h, m = both()
    good = [R.Rec(30, R.I, 80000, 16 * 100000, True), R.Rec(33, R.P, 4000, 16 * 5000, True), R.Rec(33, R.P, 4000, 16 * 5000, True)]
    lost = [R.Rec(30, R.I, -1, 16 * 100000, True), R.Rec(33, R.P, 90000, 16 * 1000, True), R.Rec(33, R.P, 90000, 16 * 1000, True)]
    for rc in (h, m):
        rc.begin_chunk(0, [3, 3])
        rc.learn([good, lost])
    same_state(h, m)
    s = h.get_state()
    assert abs(s["ratio_i"] - 0.9) < 1e-12 and abs(s["ratio_p"] - 0.9) < 1e-12                  # 0.5 x 1 + 0.5 x 0.8
    assert abs(s["rho_pi"] - (0.5 / 16 + 0.5 * 0.05 * 2 ** 0.5)) < 1e-12                        # 4000 / 80000 at QP 33 against 30


def test_measure_rho_against_the_model():
    rng = random.Random(9)
    for trial in range(200):
        h, m = both()
        n = rng.randrange(1, 7)
        qa = [rng.randrange(15, 45) for _ in range(n)]
        qt = [min(51, q + rng.randrange(0, 9)) for q in qa]
        ei = [rng.choice((0, int(16 * 10 ** rng.uniform(3, 6)))) if rng.random() < 0.2 else int(16 * 10 ** rng.uniform(3, 6)) for _ in range(n)]
        scale = (1e-4, 1.0, 1.0, 30.0)[trial % 4]                                                   # below 1/256, inside, above 1
        ep = [0 if rng.random() < 0.15 else int(e * scale * rng.uniform(0.02, 0.3)) for e in ei]
        for rc in (h, m):
            rc.measure_rho(ep, qt, ei, qa)
        same_state(h, m, trial)
        s = h.get_state()
        assert s["rho_measured"] and 1 / 256 <= s["rho_pi"] <= 1.0
        if not any(a and b for a, b in zip(ep, ei)):
            assert s["rho_pi"] == 1 / 16                                                            # nothing measured: the prior stays


def test_idr_settled_takes_the_rounded_mean_as_the_next_start():
    rng = random.Random(3)
    for trial in range(300):
        h, m = both()
        qps = [rng.randrange(18, 52) for _ in range(rng.randrange(1, 9))]
        for rc in (h, m):
            rc.begin_chunk(0, [4] * len(qps))
            rc.idr_settled(qps)
        want = math.floor(sum(qps) / len(qps) + 0.5)
        assert h.get_state()["idr_qp_hint"] == m.get_state()["idr_qp_hint"] == want
        for rc in (h, m):
            rc.begin_chunk(0, [4])
        assert h.step_qp(0, 0, []) == m.step_qp(0, 0, []) == want
    h, m = both()
    for rc in (h, m):
        rc.begin_chunk(0, [4])
    assert h.step_qp(0, 0, []) == m.step_qp(0, 0, []) == 18 + 5                                  # a session's first chunk
    assert [h.trial_qp(q) for q in (10, 48, 49, 51)] == [m.trial_qp(q) for q in (10, 48, 49, 51)] == [13, 51, 51, 51]
    assert [h.redo_idr(30, q) for q in (28, 29, 30, 31, 32)] == [m.redo_idr(30, q) for q in (28, 29, 30, 31, 32)] == [True, False, False, False, True]


# ================================================================ e. degenerate inputs
@pytest.mark.parametrize("bf", [0, 1])
@pytest.mark.parametrize("case", ["flat", "no_bits", "one_picture", "hopeless"])
def test_degenerate_inputs_stay_in_range(bf, case):
    """pictures without an estimate (flat content), CABAC sizes of 0, a GOP of one picture, a budget below one IDR picture at QP 51: every QP lies between the
    CRF's and 51, header and model agree, everything learned stays finite"""
    maxrate = 1 if case == "hopeless" else 500
    h, m = both(maxrate=maxrate, bufsize=int(1.2 * maxrate) or 1, p_slots=2)
    n = 1 if case == "one_picture" else 9
    est = 0 if case == "flat" else 16 * 200000
    for chunk in range(3):
        for rc in (h, m):
            rc.begin_chunk(bf, [n])
        qa = h.step_qp(0, 0, [])
        assert qa == m.step_qp(0, 0, []) and 18 <= qa <= 51
        want = h.want_idr(0, est, qa)
        assert want == m.want_idr(0, est, qa) and 18 <= want <= 51
        if case == "hopeless":
            assert want == 51
        for rc in (h, m):
            if n > 1 and not rc.rho_measured:
                rc.measure_rho([est // 20], [rc.trial_qp(want)], [est], [qa])
            rc.idr_settled([want])
        recs = [R.Rec(want, R.I, 0 if case == "no_bits" else est // 16, est, True)]
        types = R.step_types(bf, n)
        for t in range(1, n):
            view = visible(recs, t, 2) if types[t] == R.P else []
            qp = h.step_qp(0, t, view)
            assert qp == m.step_qp(0, t, view) and 21 <= qp <= 51, (case, t, qp)
            recs.append(R.Rec(qp, types[t], 0 if case == "no_bits" else est // 320, est // 20, True))
        for rc in (h, m):
            rc.learn([recs])
        same_state(h, m, (case, chunk))
    assert m.undecidable == 0


# ================================================================ f. closed loop
class Plant:
    """an encoder that follows the controller's own rate law: the IDR picture of lane g costs c_g x 2^(-q / 6) bits, a P picture rho times that, a B picture beta
    times a P picture at its QP less the B offset; the device estimate is 16 x bits / k"""

    def __init__(self, c, rho, beta, k, kqpb):
        self.c, self.rho, self.beta, self.k, self.kqpb = c, rho, beta, k, kqpb

    def bits(self, g, typ, qp):
        w = 1.0 if typ == R.I else self.rho if typ == R.P else self.rho * self.beta * 2 ** (self.kqpb / 6)
        return max(8, int(round(self.c[g] * w * 2 ** (-qp / 6))))

    def est(self, g, typ, qp):
        return int(round(16 * self.bits(g, typ, qp) / self.k))


def run_session(rc, plant, chunks, lanes, keyint, bf, p_slots):
    """the session's part (hevc_amd/csrc/session.cpp: encode_chunk, idr_step, rho_trial, rate_feedback, finish_rate) around a controller.  Returns per chunk
    and lane the records of the GOP in coding order, and the number of IDR analyses"""
    out, analyses = [], 0
    for chunk in range(chunks):
        glen = [keyint] * lanes
        types = R.step_types(bf, keyint)
        rc.begin_chunk(bf, glen)
        qa = [rc.step_qp(g, 0, []) for g in range(lanes)]
        ev = [plant.est(g, R.I, qa[g]) for g in range(lanes)]
        analyses += lanes
        want = [rc.want_idr(g, ev[g], qa[g]) for g in range(lanes)]
        if not rc.rho_measured and keyint > 1:
            qt = [rc.trial_qp(w) for w in want]
            rc.measure_rho([plant.est(g, R.P, qt[g]) for g in range(lanes)], qt, ev, qa)
            want = [rc.want_idr(g, ev[g], qa[g]) for g in range(lanes)]
        qps = list(qa)
        for g in range(lanes):
            if rc.redo_idr(want[g], qa[g]):
                qps[g], ev[g] = want[g], plant.est(g, R.I, want[g])
                analyses += 1
        rc.idr_settled(qps)
        recs = [[R.Rec(qps[g], R.I, plant.bits(g, R.I, qps[g]), ev[g], True)] for g in range(lanes)]
        for t in range(1, keyint):
            for g in range(lanes):
                qp = rc.step_qp(g, t, visible(recs[g], t, p_slots) if types[t] == R.P else [])
                recs[g].append(R.Rec(qp, types[t], plant.bits(g, types[t], qp), plant.est(g, types[t], qp), True))
        rc.learn(recs)
        out.append(recs)
    return out, analyses


CHUNKS, FPS, CRF = 6, 30.0, 19


def closed_loop(k, rho, lanes, keyint, bf):
    """the case's inputs: content whose uncapped rate (P pictures at crf + 2, IDR 3 below) is about four times the cap; the lanes differ by up to 1.5 x"""
    maxrate, kqpb, beta = 1000, 2, 0.45
    bufsize = int(1.2 * maxrate)                       # the reference's ratio (core/transcoder.py: bufsize = 1.2 x maxrate)
    types = R.step_types(bf, keyint)
    per_c = 2 ** (-(CRF - 1) / 6) + sum((rho if t == R.P else rho * beta) * 2 ** (-(CRF + 2) / 6) for t in types[1:])        # GOP bits at the CRF's QPs per unit of c
    c0 = 4.0 * maxrate * 1000.0 * keyint / FPS / per_c
    c = [c0 * (1.0 + 0.5 * g / max(1, lanes - 1)) for g in range(lanes)]
    args = (-1, maxrate, bufsize, 30, 1, -1, CRF - 1, CRF + 2, 1.0, 7)
    return args, Plant(c, rho, beta, k, kqpb), maxrate, bufsize


CLOSED = [(k, rho, lanes, keyint, bf) for k in (1.0, 0.7, 1.14) for rho in (1 / 32, 1 / 4) for lanes in (1, 4) for keyint in (4, 30) for bf in (0, 1)]


@functools.lru_cache(maxsize=None)
def closed_run(case):
    """the case once over the header and once over the model; what the tests below read off the header's run"""
    k, rho, lanes, keyint, bf = case
    args, plant, maxrate, bufsize = closed_loop(*case)
    h, m = Header(*args), R.Model(*args)
    got, n_h = run_session(h, plant, CHUNKS, lanes, keyint, bf, 7)
    want, n_m = run_session(m, plant, CHUNKS, lanes, keyint, bf, 7)
    # the stream in decoding order, from the second chunk on where the estimates are biased (the first has only the prior ratio)
    first = 0 if k == 1.0 else 1
    stream = [r for ch in got[first:] for lane in ch for r in lane]
    sizes, keys = [r.bits for r in stream], [r.type == R.I for r in stream]
    rate, cpb = maxrate * 1000.0, bufsize * 1000.0
    return dict(h=h, m=m, got=got, want=want, analyses=(n_h, n_m), sizes=sizes, keys=keys, rate=rate, cpb=cpb,
                slack=util.hrd_arrival_schedule(sizes, keys, rate, [int(90000 * 0.9 * cpb / rate)], FPS), mean=sum(sizes) / (len(sizes) / FPS),
                gop_share=max(sum(r.bits for r in lane) / (rate * keyint / FPS) for ch in got[first:] for lane in ch))


@pytest.mark.parametrize("k,rho,lanes,keyint,bf", CLOSED)
def test_closed_loop_header_and_model_agree_and_the_cpb_never_underflows(k, rho, lanes, keyint, bf):
    r = closed_run((k, rho, lanes, keyint, bf))
    h, m, got, want = r["h"], r["m"], r["got"], r["want"]
    assert m.undecidable == 0, "undecidable decisions: change the inputs, not the epsilon"
    assert [[[x.qp for x in lane] for lane in ch] for ch in got] == [[[x.qp for x in lane] for lane in ch] for ch in want] and r["analyses"][0] == r["analyses"][1]
    same_state(h, m)
    # conditions on the inputs: the cap binds, and the controller is never at the end of its range
    qps = [x.qp for ch in got for lane in ch for x in lane]
    p_qps = [x.qp for ch in got for lane in ch for x in lane if x.type == R.P]
    assert max(p_qps) > CRF + 2 and max(qps) < 51, (max(p_qps), max(qps))
    idr = max(s for s, key in zip(r["sizes"], r["keys"]) if key)
    print(f"k {k} rho {rho:.4f} lanes {lanes} keyint {keyint} bf {bf}: slack {r['slack'] * 1e3:.1f} ms, mean rate {r['mean'] / r['rate']:.4f} of the cap, "
          f"worst GOP {r['gop_share']:.4f} of its delivery, largest IDR {idr / r['cpb']:.3f} of the CPB, QP {min(qps)}..{max(qps)}")
    assert r["slack"] >= 0.0, f"CPB underflow by {-r['slack'] * 1e3:.1f} ms"
    assert idr <= 0.9 * r["cpb"]


# FINDING: under this plant the mean rate exceeds vbv-maxrate in 16 of the 48 cases, all of them GOPs that the IDR picture dominates (keyint 4,
# or rho 1/32) and most of them with estimates that read 14 % low (k 1.14).  Two mechanisms, both policy and not local slips: (1) want_idr takes the IDR QP
# NEAREST to the steady-state solution, which may be the one that overspends, and decide_p never plans a P picture below a quarter of an even share of the
# budget, so where P pictures are cheap (rho 1/32, keyint 4) they cannot pay an IDR picture's overdraft back and are even coded finer than planned; (2) ratio_i
# moves half way towards a chunk's measurement, so a 14 % bias is still 7 % in the second chunk and 3.5 % in the third, and an IDR-dominated GOP has nothing
# else to correct it with.  The CPB never underflows in any case (the test above).  Measured (mean rate / vbv-maxrate over the asserted part of the run):
MEAN_RATE_OVER = {(1.0, 1 / 32, 1, 4, 0): 1.0370, (1.0, 1 / 32, 1, 4, 1): 1.0249, (1.0, 1 / 32, 4, 4, 0): 1.0136, (1.0, 1 / 32, 4, 4, 1): 1.0018,
                  (1.14, 1 / 32, 1, 4, 0): 1.1639, (1.14, 1 / 32, 1, 4, 1): 1.1504, (1.14, 1 / 32, 1, 30, 0): 1.0014, (1.14, 1 / 32, 1, 30, 1): 1.0033,
                  (1.14, 1 / 32, 4, 4, 0): 1.0315, (1.14, 1 / 32, 4, 4, 1): 1.0196, (1.14, 1 / 32, 4, 30, 0): 1.0002, (1.14, 1 / 32, 4, 30, 1): 1.0018,
                  (1.14, 1 / 4, 1, 4, 0): 1.0053, (1.14, 1 / 4, 1, 4, 1): 1.0114, (1.14, 1 / 4, 4, 4, 0): 1.0084, (1.14, 1 / 4, 4, 4, 1): 1.0083}


@pytest.mark.parametrize("k,rho,lanes,keyint,bf", [pytest.param(*c, marks=pytest.mark.xfail(strict=True, reason=f"measured mean rate {MEAN_RATE_OVER[c]:.4f} x vbv-maxrate: DESIGN.md §9"))
                                                   if c in MEAN_RATE_OVER else c for c in CLOSED])
def test_closed_loop_mean_rate_stays_under_the_cap(k, rho, lanes, keyint, bf):
    r = closed_run((k, rho, lanes, keyint, bf))
    assert r["mean"] <= r["rate"], f"mean rate {r['mean'] / r['rate']:.4f} of the cap, worst GOP {r['gop_share']:.4f} of its delivery"
