"""Inverse telecine of DESIGN.md §6h (mihevc_send_frame_fieldmatch / mihevc_k_fieldmatch_metrics / mihevc_k_fieldmatch_weave) as a numpy model, written from the
definition and not from the kernels: no tiles, no runs, no staging; whole planes of Python ints (int64).  metrics() and weave() are the two kernels, plan() the
host's decisions, pictures() the sequence rules of a session.  scalar_metrics() restates the metrics sample by sample in plain Python."""
import numpy as np

from tests import deint_ref as D

COMB_T, COMB_BLOCK, CYCLE = 9, 80, 5
ONES64, ONES32 = (1 << 64) - 1, (1 << 32) - 1
coded, dtype = D.coded, D.dtype


def _clamped(p, depth):
    return np.minimum(np.asarray(p).astype(np.int64), (1 << depth) - 1)


def weave_plane(C, X, keep):
    """rows of parity keep from C, the others from X"""
    out = np.array(X, copy=True)
    out[keep::2] = C[keep::2]
    return out


def _block_max(a, bh, bw):
    """the largest sum of `a` over any bh x bw block of the grid anchored at (0, 0); partial blocks count what they have"""
    H, W = a.shape
    pad = np.zeros((-(-H // bh) * bh, -(-W // bw) * bw), np.int64)
    pad[:H, :W] = a
    return int(pad.reshape(pad.shape[0] // bh, bh, pad.shape[1] // bw, bw).sum(axis=(1, 3)).max())


def comb_map(Wm, depth):
    """(combed, strength) of a woven luma plane; rows 0 and H - 1 are never combed"""
    T = COMB_T << (depth - 8)
    d1, d2 = Wm[:-2] - Wm[1:-1], Wm[2:] - Wm[1:-1]
    inner = ((d1 > T) & (d2 > T)) | ((d1 < -T) & (d2 < -T))
    combed = np.zeros(Wm.shape, bool)
    combed[1:-1] = inner
    strength = np.zeros(Wm.shape, np.int64)
    strength[1:-1] = np.where(inner, np.minimum(np.abs(d1), np.abs(d2)), 0)
    return combed, strength


def metrics(P, C, N, depth, keep):
    """luma planes of three frames -> [S_c, S_p, S_n, K_c, K_p, K_n, DS, DB] as the kernel takes them (no first-frame rule)"""
    P, C, N = (_clamped(p, depth) for p in (P, C, N))
    H, W = C.shape
    assert W >= 16 and H >= 16 and W % 2 == 0 and H % 4 == 0 and keep in (0, 1)
    S, K = [], []
    for X in (C, P, N):
        combed, strength = comb_map(weave_plane(C, X, keep), depth)
        S.append(int(strength.sum()))
        K.append(_block_max(combed.astype(np.int64), 16, 16))
    q = np.zeros((H, W), np.int64)
    q[keep::2] = np.abs(C[keep::2] - P[keep::2])
    return S + K + [int(q.sum()), _block_max(q, 32, 32)]


def scalar_metrics(P, C, N, depth, keep):
    """the same numbers, one sample at a time, as DESIGN.md §6h words them"""
    peak, T = (1 << depth) - 1, COMB_T << (depth - 8)
    P, C, N = ([[min(int(v), peak) for v in row] for row in p] for p in (P, C, N))
    H, W = len(C), len(C[0])
    out_s, out_k = [], []
    for X in (C, P, N):
        Wm = [C[y] if (y & 1) == keep else X[y] for y in range(H)]
        total, blocks = 0, {}
        for y in range(1, H - 1):
            for x in range(W):
                d1, d2 = Wm[y - 1][x] - Wm[y][x], Wm[y + 1][x] - Wm[y][x]
                if (d1 > T and d2 > T) or (d1 < -T and d2 < -T):
                    total += min(abs(d1), abs(d2))
                    blocks[(y // 16, x // 16)] = blocks.get((y // 16, x // 16), 0) + 1
        out_s.append(total)
        out_k.append(max(blocks.values(), default=0))
    ds, blocks = 0, {}
    for y in range(keep, H, 2):
        for x in range(W):
            q = abs(C[y][x] - P[y][x])
            ds += q
            blocks[(y // 32, x // 32)] = blocks.get((y // 32, x // 32), 0) + q
    return out_s + out_k + [ds, max(blocks.values(), default=0)]


def weave(cur, other, depth, keep):
    """cur / other: (Y, Cb, Cr), display size -> [Y, Cb, Cr] of the coded size, values clamped, margin by ingest.h's rule"""
    H, W = cur[0].shape
    pw, ph = coded(W), coded(H)
    out = []
    for i in range(3):
        o = weave_plane(_clamped(cur[i], depth), _clamped(other[i], depth), keep)
        out.append(np.ascontiguousarray(D.with_margin(o, pw if i == 0 else pw // 2, ph if i == 0 else ph // 2).astype(dtype(depth))))
    return out


def plan(mets, decimate, deint):
    """mets: per frame the eight numbers of metrics() -> per frame dict(metrics (first-frame rule applied), match, deinterlaced, dropped, picture)"""
    frames = []
    for k, m in enumerate(mets):
        m = list(m)
        if k == 0:
            m[6], m[7] = ONES64, ONES32
        match = min(range(3), key=lambda i: (m[i], i))
        frames.append(dict(metrics=m, match=match, deinterlaced=bool(deint and m[3 + match] > COMB_BLOCK), dropped=False, picture=-1))
    pictures = 0
    for k0 in range(0, len(frames), CYCLE):
        cyc = frames[k0:k0 + CYCLE]
        drop = min(range(CYCLE), key=lambda i: (cyc[i]["metrics"][7], cyc[i]["metrics"][6], i)) if decimate and len(cyc) == CYCLE else -1
        for i, f in enumerate(cyc):
            f["dropped"] = i == drop
            if i != drop:
                f["picture"] = pictures
                pictures += 1
    return frames


def pictures(frames, depth, tff=True, decimate=True, deint=True):
    """the sequence rules of a session for frames sent with pts = i: ([(pts, [Y, Cb, Cr] of the coded size)], the plan).  With decimate the j-th picture takes
    pts j"""
    keep = 0 if tff else 1
    n = len(frames)
    nb = [(frames[max(k - 1, 0)], frames[k], frames[min(k + 1, n - 1)]) for k in range(n)]
    decided = plan([metrics(P[0], C[0], N[0], depth, keep) for P, C, N in nb], decimate, deint)
    out = []
    for k, (f, (P, C, N)) in enumerate(zip(decided, nb)):
        if f["dropped"]:
            continue
        pic = D.deinterlace(P, C, N, depth, keep, 0)[0] if f["deinterlaced"] else weave(C, (C, P, N)[f["match"]], depth, keep)
        out.append((f["picture"] if decimate else k, pic))
    return out, decided
