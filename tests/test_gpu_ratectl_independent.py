"""GPU (-m gpu): real sessions under a binding cap whose every QP the independent rate-control model (tests/ratectl_ref.py) must predict from outside.

A session shows QP, slice type and CABAC size per picture (frame_info) but not the rate estimates its controller steers by.  The oracle produces the same
estimate (Analysis.est), so the estimates are REBUILT: every P and B estimate at the session's QP against the session's own reconstructions (keep_recon), every
IDR estimate at the QP of its first analysis and, after a second analysis, at its final QP, and in a session's first chunk the trial estimate (each GOP's first
P picture at trial_qp(wanted) against the UNFILTERED reconstruction of the IDR analysis, without the intra second pass, with the pre-search centres).  The model
is then driven with those numbers and the session's CABAC sizes in the session's order (begin_chunk, step 0, the lags of §5b through test_ratectl_cpu.visible,
learn), and its QP for every picture must be frame_info's.  The number of IDR analyses the model went through must be the session's (profile_stages 1:
stats.stage_launches[0] counts the launches, one per chunk plus one per chunk that analysed lanes again; stats.stage_pictures[0] the pictures in them: first
analyses plus lanes analysed again).  Estimate parity between the device's stage entries and the oracle is asserted first, for one IDR and one P picture per
case, so that a divergence reads as a parity fault and not as a policy fault.

Out of scope: sliced sessions (estimates summed over the bands of a picture): the oracle has no per-band IDR analysis to rebuild their estimates from.

The cases, their caps and the measured rates the caps come from stand next to CASES below.
"""
import importlib.util
from pathlib import Path

import pytest

from oracle import oracle as O
from tests import ratectl_ref as R
from tests import util
from tests.test_gpu_configs import session_params
from tests.test_ratectl_cpu import visible

pytestmark = pytest.mark.gpu

CRF = 20
# The caps follow the method of tests/golden/make_step0_goldens.py --scan: the clip's rate at its CRF with the cap off (measured on an MI355X at 30 pictures a
# second, kb/s), then the stated fraction of it.  The noise case takes the cap of the step-0 fixture: a tenth of what white noise takes at CRF 20.
CRF_RATE = {"carry": 1064, "bpic": 355, "ring8": 280, "ring12": 280, "ring12k16": 268}
CAP = {k: v // 3 for k, v in CRF_RATE.items()}
# name: (width, height, bit depth, keyint, lanes, pictures, bframes, level_idc, content, cap kb/s)
CASES = {
    # the hint carried across chunks, learn feeding the next chunk, a flushed last chunk of equalised GOPs (4 + 4)
    "carry": (256, 128, 8, 6, 4, 80, 0, 93, "texture", CAP["carry"]),
    # the noise_redo inputs of make_step0_goldens.py over 2 chunks: the trial, then every lane analysed again
    "redo": (256, 128, 8, 4, 4, 32, 0, 93, "noise", 1600),
    # beta_bp, B QPs, display positions in the records, a size off the CTU grid, Main10
    "bpic": (136, 72, 10, 5, 2, 30, 1, 93, "texture", CAP["bpic"]),
    # one lane, the ring at its smallest (8 slots below level 5: CABAC sizes 7 steps late) and at its largest (12 from level 5 on: 11 steps late, which a GOP
    # of 12 never sees; a GOP of 16 does)
    "ring8": (96, 80, 8, 12, 1, 24, 0, 93, "texture", CAP["ring8"]),
    "ring12": (96, 80, 8, 12, 1, 24, 0, 150, "texture", CAP["ring12"]),
    "ring12k16": (96, 80, 8, 16, 1, 32, 0, 150, "texture", CAP["ring12k16"]),
}


def _step0_maker():
    spec = importlib.util.spec_from_file_location("make_step0_goldens", Path(__file__).parent / "golden" / "make_step0_goldens.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def lib():
    from hevc_amd import _lib
    L = _lib.load()
    assert L.mihevc_device_count() >= 1, "no gfx950 device visible: the GPU tests need an MI355X"
    return L


def config(name, cap=None):
    from hevc_amd import _lib
    w, h, bd, keyint, lanes, n, bframes, level, content, case_cap = CASES[name]
    cap = case_cap if cap is None else cap
    cfg = _lib.default_config()
    cfg.width, cfg.height, cfg.bit_depth, cfg.keyint, cfg.min_keyint, cfg.gops_in_flight, cfg.scenecut, cfg.me_range, cfg.level_idc = w, h, bd, keyint, 2, lanes, 0, 8, level
    cfg.crf, cfg.qp, cfg.vbv_maxrate_kbps, cfg.vbv_bufsize_kbits, cfg.profile_stages, cfg.bframes = CRF, -1, cap, cap * 6 // 5, 1, bframes
    return cfg


def clip(name):
    w, h, bd, keyint, lanes, n, bframes, level, content, cap = CASES[name]
    if content == "noise":
        M = _step0_maker()
        assert (M.W, M.H, M.KEYINT) == (w, h, keyint) and M.CASES["noise_redo"][2:6] == (lanes, CRF, cap, cap * 6 // 5)
        return [util.to_frame(M.picture("noise", i)) for i in range(n)]
    return [util.synth_frame(h, w, seed=9, shift=(2 * i, i), bit_depth=bd) for i in range(n)]          # (synth_frame has room for shifts up to 190 samples)


def run_session(cfg, frames):
    from hevc_amd.encoder import Encoder
    n, bd = len(frames), cfg.bit_depth
    with Encoder(cfg, device=0, keep_recon=True) as enc:
        for f in frames:
            enc.send(*util.planes(f, bd))
        enc.flush()
        packets = list(enc.packets_dts())
        infos = [enc.frame_info(i) for i in range(n)]
        recs = [O.Frame(*enc.recon(i)) for i in range(n)]
        st = enc.stats()
    assert len(packets) == n
    return infos, recs, st


def chunks_of(n, keyint, lanes):
    """(first picture, GOP lengths) per chunk of a session without scene cuts: lanes x keyint pictures a chunk, the flushed rest as the fewest GOPs of near-equal
    length (util.idr_positions states the same; asserted against the session's IDR pictures)"""
    out, pos = [], 0
    while pos < n:
        m = min(lanes * keyint, n - pos)
        g = (m + keyint - 1) // keyint
        out.append((pos, [m // g + (j < m % g) for j in range(g)]))
        pos += m
    return out


class Estimates:
    """the oracle's rate estimates of a session's pictures, rebuilt from its sources and reconstructions"""

    def __init__(self, lib, cfg, frames, infos, recs):
        self.lib, self.cfg, self.frames, self.infos, self.recs, self.bd = lib, cfg, frames, infos, recs, cfg.bit_depth
        self.intra_cache = {}

    def centres(self, i, ref_i):
        return O.search_centres(self.frames[i], self.frames[ref_i], self.bd) if self.cfg.pre_search else None

    def intra(self, i, qp):
        if (i, qp) not in self.intra_cache:
            self.intra_cache[(i, qp)] = O.analyze_intra(self.frames[i], session_params(self.lib, self.cfg, qp, True)[0])
        return self.intra_cache[(i, qp)]

    def p(self, i, ref_i):
        prm, _ = session_params(self.lib, self.cfg, self.infos[i][0], False)
        return O.analyze_inter(self.frames[i], self.recs[ref_i], prm, centers=self.centres(i, ref_i)).est

    def b(self, i):
        prm, _ = session_params(self.lib, self.cfg, self.infos[i][0], False)
        return O.analyze_b(self.frames[i], self.recs[i - 1], self.recs[i + 1], prm, self.centres(i, i - 1), self.centres(i, i + 1)).est

    def trial(self, i, idr_i, qa, qp):
        """the rho trial: picture i at qp against the unfiltered reconstruction of the IDR analysis at qa; the inter pass alone"""
        prm, _ = session_params(self.lib, self.cfg, qp, False)
        prm.intra_in_p = 0
        return O.analyze_inter(self.frames[i], self.intra(idr_i, qa).rec, prm, centers=self.centres(i, idr_i)).est


def audit(lib, cfg, frames, infos, recs, st):
    """drives the model through the session; returns (model, decisions left to the session, launches and pictures of the IDR stage, lanes analysed again per chunk)"""
    n, bf = len(frames), cfg.bframes > 0
    lanes = cfg.gops_in_flight
    p_slots = (12 if cfg.level_idc >= 150 else 8) - 1
    m = R.Model(cfg.qp, cfg.vbv_maxrate_kbps, cfg.vbv_bufsize_kbits, cfg.fps_num, cfg.fps_den, cfg.b_qp_offset, CRF - 1, CRF + 2, 1.0, p_slots)
    E = Estimates(lib, cfg, frames, infos, recs)
    chunks = chunks_of(n, cfg.keyint, lanes)
    assert [i for i, (_, t, _) in enumerate(infos) if t == R.I] == util.idr_positions(n, cfg.keyint, lanes) == [s + sum(gl[:g]) for s, gl in chunks for g in range(len(gl))]
    launches = pictures = skipped = 0
    redone = []                         # per chunk: lanes analysed a second time
    for start, glen in chunks:
        B = len(glen)
        g0 = [start + sum(glen[:g]) for g in range(B)]
        tables = [R.gop_table(bf, k) for k in glen]
        m.begin_chunk(bf, glen)
        # ---- step 0
        before = m.undecidable
        qa = [m.step_qp(g, 0, []) for g in range(B)]
        ev = [E.intra(g0[g], qa[g]).est for g in range(B)]
        launches, pictures = launches + 1, pictures + B
        want = [m.want_idr(g, ev[g], qa[g]) for g in range(B)]
        first_p = sum(1 for k in glen if k > 1)
        if not m.rho_measured and glen[0] > 1 and first_p:
            qt = [m.trial_qp(want[g]) for g in range(first_p)]
            ep = [E.trial(g0[g] + tables[g][1].pos, g0[g], qa[g], qt[g]) for g in range(first_p)]
            m.measure_rho(ep, qt, ev, qa)
            want = [m.want_idr(g, ev[g], qa[g]) for g in range(B)]
        qps, redo = list(qa), [g for g in range(B) if m.redo_idr(want[g], qa[g])]
        for g in redo:
            qps[g], ev[g] = want[g], E.intra(g0[g], want[g]).est
        if m.undecidable > before:          # a decision of step 0 on a threshold: the session's word stands
            skipped += m.undecidable - before
            redo = [g for g in range(B) if infos[g0[g]][0] != qa[g]]
            for g in range(B):
                qps[g] = infos[g0[g]][0]
                ev[g] = E.intra(g0[g], qps[g]).est
        if redo:
            launches, pictures = launches + 1, pictures + len(redo)
        redone.append(len(redo))
        assert qps == [infos[i][0] for i in g0], (start, "IDR QPs", qps, [infos[i][0] for i in g0], qa, want, ev)
        m.idr_settled(qps)
        lane = [[R.Rec(qps[g], R.I, infos[g0[g]][2], ev[g], True)] for g in range(B)]
        # ---- the P and B steps, lanes in lock-step
        for t in range(1, glen[0]):
            for g in range(B):
                if t >= glen[g]:
                    continue
                pic = tables[g][t]
                i = g0[g] + pic.pos
                qp_s, type_s, bits_s = infos[i]
                assert type_s == pic.type, (i, type_s, pic)
                before = m.undecidable
                qp = m.step_qp(g, t, visible(lane[g], t, p_slots) if pic.type == R.P else [])
                if m.undecidable > before:
                    skipped += 1
                    qp = m.anchor_qp[g] = qp_s
                assert qp == qp_s, (f"picture {i} (chunk at {start}, lane {g}, step {t}, type {pic.type}): model {qp}, session {qp_s}", m.decisions[-1], m.get_state())
                est = E.p(i, g0[g] + pic.refs[0]) if pic.type == R.P else E.b(i)
                lane[g].append(R.Rec(qp, pic.type, bits_s, est, True))
        m.learn(lane)
    return m, skipped, launches, pictures, redone


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_model_predicts_every_qp_of_a_session(lib, name):
    cfg, frames = config(name), clip(name)
    infos, recs, st = run_session(cfg, frames)
    assert st.frames_out == len(frames)
    # estimate parity first: the stage entries against the oracle, the first IDR picture and the first P picture at the session's QPs
    api = util.StageApi(lib, "mihevc_k_", device=0)
    E = Estimates(lib, cfg, frames, infos, recs)
    _, cp = session_params(lib, cfg, infos[0][0], True)
    assert api.intra(frames[0], cp).est == E.intra(0, infos[0][0]).est, "IDR estimate: the stage entry and the oracle differ"
    p1 = R.gop_table(cfg.bframes > 0, cfg.keyint)[1].pos
    _, cp = session_params(lib, cfg, infos[p1][0], False)
    assert api.inter(frames[p1], recs[0], cp, centers=E.centres(p1, 0)).est == E.p(p1, 0), "P estimate: the stage entry and the oracle differ"
    # the policy
    m, skipped, launches, pictures, redone = audit(lib, cfg, frames, infos, recs, st)
    assert skipped <= 1, f"{skipped} decisions on a threshold: choose other content"
    assert (int(st.stage_launches[0]), int(st.stage_pictures[0])) == (launches, pictures), "IDR analyses: the model went another way through step 0"
    p_qps = [q for q, t, _ in infos if t == R.P]
    assert max(p_qps) > CRF + 2, "the cap did not bind: the test would pass on a controller that never acts"
    if name == "redo":
        assert redone[0] == cfg.gops_in_flight and len(redone) == 2, "the noise case: every lane of the first chunk is analysed twice"
    if name == "bpic":
        assert m.beta_bp != 0.45 and any(t == R.B for _, t, _ in infos)
