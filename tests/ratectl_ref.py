"""The rate-control policy of a session (the comments of hevc_amd/csrc/ratectl.h and include/mihevc.h) as a second, independent statement in
plain Python: what the controller is SAID to do, written from the prose, not from the method bodies (tests/test_ratectl_cpu.py holds the header against it on
arrays, tests/test_gpu_ratectl_independent.py whole sessions).

Imports: the standard library only (math, collections).  Nothing of hevc_amd/, oracle/ or the other test modules (tests/test_syntax_independent.py checks that).

Structure, different from the header's on purpose:
  * a GOP is first laid out as a SIMULATION of its reconstruction buffers (`gop_table`): display order is typed, coding order is derived from "a B picture is
    coded right behind the later of its two anchors", and every picture is put into a buffer that nothing still needs;
  * a P decision first CLASSIFIES every earlier step of the GOP by what is known about it at step t (its CABAC size, its device estimate, or nothing: the model),
    then prices the GOP from that table (`Model.p_decision`);
  * the IDR decision ENUMERATES its candidates into a list and takes the first minimum (`Model.idr_candidates`, `Model.want_idr`).

Floating point: float64 throughout, as the header.  Every decision also reports how far it was from the nearest point where it would have come out differently
(`Decision.margin`: the 0.75 dead band, the halves where a rounding flips, the gap between the two best IDR candidates).  A decision with a margin below EPS
is "undecidable": the last place of exp2 / log2 may differ between two libraries, so a comparison leaves it out (Model.undecidable counts them)."""
import collections
import math

EPS = 1e-9                      # margin below which a decision is undecidable
IDR_START = 5                   # a session's first chunk analyses its IDR pictures this far above the CRF's IDR QP
IDR_REDO = 2                    # an IDR picture is analysed again when the wanted QP is at least this far from the analysed one
BUDGET_SHARE = 0.985            # a GOP is planned to this share of vbv-maxrate x its duration
CPB_START, IDR_CPB_SHARE = 0.9, 0.85      # CPB fullness a GOP may assume at its IDR, and the share of it the IDR picture may take
I_P_OFFSET = 3                  # steady P QP the IDR decision aims at, above the IDR QP
DEAD_BAND = 0.75
I, P, B = 2, 1, 0               # slice types as frame_info reports them

Rec = collections.namedtuple("Rec", "qp type bits est est_known", defaults=(0, 0, -1, 0, False))      # bits < 0: no CABAC size; est: 1/16 bit
Decision = collections.namedtuple("Decision", "qp margin detail")
Picture = collections.namedtuple("Picture", "pos type cur refs")      # one coding step: display position, type, buffer written, display positions predicted from


# ================================================================ GOP structure
def display_types(bf, length):
    """the GOP in display order: an IDR picture, then P pictures; with B pictures every second picture is an anchor, the LAST one always is, and a B picture
    sits only between two anchors"""
    types = [I] + [P] * (length - 1)
    if bf:
        for pos in range(1, length - 1, 2):
            types[pos] = B
    return types


def gop_table(bf, length):
    """coding order by simulation: walk the anchors in display order; each is coded, then the B picture it closes (the one between it and the anchor before).
    Buffers: three, as the session has.  A picture goes into a buffer whose content no later step reads; an anchor never into the one the previous anchor
    holds.  Returns the steps as Picture tuples."""
    types = display_types(bf, length)
    anchors = [p for p in range(length) if types[p] != B]
    holds, steps = {}, []                        # buffer -> display position it holds

    def free_buffer(needed):
        for b in (0, 1, 2):
            if holds.get(b) not in needed:
                return b
        raise AssertionError("three buffers do not suffice")

    for k, a in enumerate(anchors):
        before = anchors[k - 1] if k else None
        refs = () if before is None else (before,)
        between = [p for p in range((before if before is not None else 0) + 1, a)]
        # what must survive this step: the reference, and (for the B picture coded next) this anchor's predecessor
        cur = free_buffer(set(refs))
        holds[cur] = a
        steps.append(Picture(a, types[a], cur, refs))
        for bpos in between:
            assert types[bpos] == B
            cur = free_buffer({before, a})
            holds[cur] = bpos
            steps.append(Picture(bpos, B, cur, (before, a)))
    assert len(steps) == length
    return steps


def step_types(bf, length):
    return [s.type for s in gop_table(bf, length)]


# ================================================================ rounding and the walk, with margins
def round_half_away(x):
    """(nearest integer, halves away from zero; distance of x to the nearest half)"""
    r = math.floor(abs(x) + 0.5)
    return int(math.copysign(r, x)), abs(abs(x) - math.floor(abs(x)) - 0.5)


WALK = ((-math.inf, -DEAD_BAND, -1), (-DEAD_BAND, DEAD_BAND, 0), (DEAD_BAND, 1.5, 1), (1.5, 2.5, 2), (2.5, math.inf, 3))


def walk_step(d):
    """the controller moves towards the QP it solved for: -1 per picture when it is 0.75 or more below, not at all inside the dead band, else by the rounded
    distance, +3 at the most.  Intervals are closed towards the move.  Returns (move, distance of d to the nearest interval end)."""
    margin = min(abs(d - e) for lo, hi, _ in WALK for e in (lo, hi) if math.isfinite(e))
    if d <= -DEAD_BAND:
        return -1, margin
    for lo, hi, move in WALK[1:]:
        if d < hi:
            return move, margin
    raise AssertionError(d)


def log2_ratio(num, den):
    """log2(num / den) where a zero numerator is minus infinity (a picture with no estimate), den > 0"""
    return -math.inf if num <= 0 else math.log2(num / den)


class Model:
    """One controller per session; the lanes of a chunk are independent but for the learned state.  Calls mirror what a session does:
    begin_chunk, step_qp per lane and step, at step 0 want_idr / (first chunk) measure_rho / idr_settled, learn behind the chunk."""

    def __init__(self, qp_cfg, maxrate_kbps, bufsize_kbits, fps_num, fps_den, b_qp_offset, qp_i, qp_p, share, p_slots):
        self.on = qp_cfg < 0 and maxrate_kbps > 0                     # rate control: CRF mode with a cap
        self.rate = share * maxrate_kbps * 1000.0                     # this session's part of the channel, bits per second
        self.idr_cap = IDR_CPB_SHARE * CPB_START * share * bufsize_kbits * 1000.0 if bufsize_kbits > 0 else math.inf
        self.fps = fps_num / fps_den
        self.qp_i, self.qp_p, self.p_slots = qp_i, qp_p, p_slots
        self.b_offset = min(8, b_qp_offset) if b_qp_offset >= 0 else 2
        # learned
        self.ratio_i = self.ratio_p = 1.0
        self.rho_pi, self.beta_bp = 1.0 / 16.0, 0.45
        self.idr_qp_hint, self.rho_measured = -1, False
        self.undecidable = 0
        self.decisions = []

    # ---------------------------------------------------------------- chunk
    def begin_chunk(self, bf, glen):
        self.bf, self.glen = bool(bf), list(glen)
        self.types = [step_types(self.bf, n) for n in glen]
        self.budget = [BUDGET_SHARE * self.rate * n / self.fps for n in glen]
        self.anchor_qp = [self.qp_p] * len(glen)

    def weight(self, typ):
        """a picture in units of a P picture"""
        return 1.0 if typ == P else self.beta_bp

    def note(self, dec):
        self.decisions.append(dec)
        if dec.margin < EPS:
            self.undecidable += 1
        return dec

    def step_qp(self, g, t, recs):
        typ = self.types[g][t]
        if typ == I:
            start = self.qp_i if not self.on else (self.idr_qp_hint if self.idr_qp_hint >= 0 else self.qp_i + IDR_START)
            dec = Decision(min(51, max(self.qp_i, start)), math.inf, "idr start")
        elif typ == B:
            return self.note(Decision(min(51, self.anchor_qp[g] + self.b_offset), math.inf, "b")).qp       # leaves the walk alone
        elif not self.on:
            dec = Decision(self.qp_p, math.inf, "crf")
        else:
            dec = self.p_decision(g, t, recs)
        self.anchor_qp[g] = dec.qp
        return self.note(dec).qp

    # ---------------------------------------------------------------- P pictures
    def classify(self, g, t, recs):
        """what is known at step t about each step 1 <= j < t: 'size' (its CABAC job is done for sure: its ring slot has been handed out again, p_slots steps
        later), 'estimate' (the device estimate is read with a lag of two steps; a finished CABAC job brings it too), or 'model'"""
        table = {}
        for j in range(1, t):
            r = recs[j]
            size = r.bits if j <= t - self.p_slots and r.bits >= 0 else None
            landed = r.est if j <= t - 2 and r.est_known else None
            table[j] = dict(type=self.types[g][j], qp=r.qp, size=size, landed=landed,
                            paired=r.est if size is not None and r.est > 0 else None,
                            kind="size" if size is not None else "estimate" if landed is not None else "model")
        return table

    def p_decision(self, g, t, recs):
        table, n, budget = self.classify(g, t, recs), self.glen[g], self.budget[g]
        # 1. CABAC bits per estimated bit in this GOP: the finished pictures, and two pictures' worth of the session's ratio at the size of the latest
        #    estimate that landed with something in it
        pairs = [(e["size"], e["paired"] / 16.0) for e in table.values() if e["paired"] is not None]
        landed = [e["landed"] for j, e in sorted(table.items(), reverse=True) if e["landed"]]
        seed = 2.0 * landed[0] / 16.0 if landed else 0.0
        num, den = sum(b for b, _ in pairs) + self.ratio_p * seed, sum(e for _, e in pairs) + seed
        ratio = num / den if den > 0 else self.ratio_p
        # 2. the rate model's reference point: geometric mean of the last two landed P estimates brought to the later one's QP, else the IDR prior
        idr_bits = recs[0].est / 16.0 * self.ratio_i
        last_p = [e for j, e in sorted(table.items(), reverse=True) if e["type"] == P and e["landed"] is not None][:2]
        if last_p:
            q_ref = last_p[0]["qp"]
            b_ref = 2.0 ** (sum(math.log2(max(1.0, e["landed"] / 16.0 * ratio)) + (e["qp"] - q_ref) / 6.0 for e in last_p) / len(last_p))
        else:
            q_ref, b_ref = recs[0].qp, idr_bits * self.rho_pi

        def modelled(e):       # a P picture at its QP; a B picture as beta x a P picture at its QP less the B offset
            q = e["qp"] - (self.b_offset if e["type"] == B else 0)
            return self.weight(e["type"]) * b_ref * 2.0 ** ((q_ref - q) / 6.0)
        price = {"size": lambda e: float(e["size"]), "estimate": lambda e: e["landed"] / 16.0 * ratio, "model": modelled}
        spent = idr_bits + sum(price[e["kind"]](e) for _, e in sorted(table.items()))
        # 3. the constant QP that spends what is left over the pictures to come (never planning below a quarter of an even share)
        to_come = sum(self.weight(typ) for typ in self.types[g][t:n])
        target = max((budget - spent) / max(0.5, to_come), 0.25 * budget / n)
        q_ss = q_ref + 6.0 * log2_ratio(b_ref, target)
        if t == 1:             # the first P picture goes straight to the model, never finer than its IDR
            if q_ss == -math.inf:
                qp, margin = recs[0].qp, math.inf
            else:
                qp, margin = round_half_away(q_ss)
                qp = max(qp, recs[0].qp)
        else:
            move, margin = walk_step(q_ss - self.anchor_qp[g])
            qp = self.anchor_qp[g] + move
        return Decision(min(51, max(self.qp_p, qp)), margin, dict(q_ss=q_ss, ratio=ratio, b_ref=b_ref, q_ref=q_ref, spent=spent, target=target))

    # ---------------------------------------------------------------- IDR pictures
    def idr_size(self, est, qa, q):
        """modelled size of an IDR picture at QP q from its estimate at QP qa"""
        return max(1.0, est / 16.0 * self.ratio_i) * 2.0 ** ((qa - q) / 6.0)

    def idr_candidates(self, g, est, qa):
        """(qp, rank, distance): rank 0 candidates are real ones, rank 1 what is left when nothing fits (then the smallest picture wins)"""
        n, budget, out = self.glen[g], self.budget[g], []
        others = sum(self.weight(typ) for typ in self.types[g][1:n])
        for q in range(self.qp_i, 52):
            size = self.idr_size(est, qa, q)
            if size > self.idr_cap and q < 51:
                continue
            left = budget - size
            if n < 2:
                out.append((q, 0, float(q)) if size <= budget else (q, 1, size))      # IDR-only GOP: the finest QP that fits
            elif left <= 0:
                out.append((q, 1, size))
            else:                                                                     # steady P QP this IDR QP leads to, against IDR QP + 3
                steady = max(float(self.qp_p), q + 6.0 * math.log2(size * self.rho_pi / (left / max(0.5, others))))
                out.append((q, 0, abs(steady - (q + I_P_OFFSET))))
        return out

    def want_idr(self, g, est, qa):
        cands = self.idr_candidates(g, est, qa)
        rank = min(r for _, r, _ in cands)
        pool = [(q, d) for q, r, d in cands if r == rank]
        best = min(d for _, d in pool)
        pick = next(q for q, d in pool if d == best)
        margin = min([abs(d - best) for q, d in pool if q != pick] or [math.inf])
        # a candidate that only just fits (or only just misses) the IDR cap or the budget
        edges = [abs(self.idr_size(est, qa, q) - lim) / lim for q in range(self.qp_i, 52) for lim in (self.idr_cap, self.budget[g]) if math.isfinite(lim)]
        margin = min([margin] + edges)
        return self.note(Decision(pick, margin, "idr")).qp

    @staticmethod
    def trial_qp(want):
        return min(51, want + I_P_OFFSET)

    @staticmethod
    def redo_idr(want, qa):
        return abs(want - qa) >= IDR_REDO

    def measure_rho(self, est_p, qp_trial, est_i, qa):
        """first chunk: P / IDR size ratio at equal QP from the trial estimates, geometric mean over the lanes that have both"""
        logs = [math.log2(ep / ei) + (qt - q) / 6.0 for ep, qt, ei, q in zip(est_p, qp_trial, est_i, qa) if ep and ei]
        if logs:
            self.rho_pi = min(1.0, max(1.0 / 256, 2.0 ** (sum(logs) / len(logs))))
        self.rho_measured = True

    def idr_settled(self, qps):
        for g, q in enumerate(qps):
            self.anchor_qp[g] = q
        self.idr_qp_hint = (2 * sum(qps) + len(qps)) // (2 * len(qps))       # mean, halves up

    # ---------------------------------------------------------------- behind a chunk
    def learn(self, lanes):
        """every picture of the chunk that has a size and an estimate, in a lane whose IDR picture has both, becomes one sample: (type, bits, estimated bits,
        log2 of its size against the IDR picture's with both brought to one QP; a B picture first to the QP of its anchors)"""
        samples = []
        for g, recs in enumerate(lanes):
            idr = recs[0]
            if idr.bits < 0 or not idr.est:
                continue
            samples.append((I, float(idr.bits), idr.est / 16.0, 0.0))
            for j in range(1, self.glen[g]):
                r, typ = recs[j], self.types[g][j]
                if r.bits > 0 and r.est:
                    q = r.qp - (self.b_offset if typ == B else 0)
                    samples.append((typ, float(r.bits), r.est / 16.0, (math.log2(r.bits / idr.bits) if idr.bits else math.inf) + (q - idr.qp) / 6.0))

        def total(types, k):
            return sum(s[k] for s in samples if s[0] in types)
        if total((I,), 2) > 0:
            self.ratio_i = 0.5 * self.ratio_i + 0.5 * total((I,), 1) / total((I,), 2)
        if total((P, B), 2) > 0:
            self.ratio_p = 0.5 * self.ratio_p + 0.5 * total((P, B), 1) / total((P, B), 2)
        n_p, n_b = sum(s[0] == P for s in samples), sum(s[0] == B for s in samples)
        if n_p:
            mean_p = total((P,), 3) / n_p
            self.rho_pi = min(1.0, max(1.0 / 256, 0.5 * self.rho_pi + 0.5 * 2.0 ** mean_p))
            if n_b:
                self.beta_bp = min(1.5, max(0.05, 0.5 * self.beta_bp + 0.5 * 2.0 ** (total((B,), 3) / n_b - mean_p)))

    # ---------------------------------------------------------------- state
    def get_state(self):
        return dict(ratio_i=self.ratio_i, ratio_p=self.ratio_p, rho_pi=self.rho_pi, beta_bp=self.beta_bp, idr_qp_hint=self.idr_qp_hint, rho_measured=self.rho_measured)

    def set_state(self, **kw):
        for k, v in kw.items():
            assert k in ("ratio_i", "ratio_p", "rho_pi", "beta_bp", "idr_qp_hint", "rho_measured"), k
            setattr(self, k, v)
