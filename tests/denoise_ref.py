"""The denoiser of DESIGN.md §6g (mihevc_send_frame_denoise / mihevc_k_denoise) as a numpy model, written from the definition and not from the kernel: no tiles, no
runs, no staging, no packed sums and no reciprocal; whole planes of int64, one statement per line of the definition, the division numpy's own floor division.
denoise() returns the three planes of the CODED size and one Counter of weight classes per plane; the sequence rules of a session are in pictures()."""
import collections

import numpy as np

from tests.deint_ref import coded, dtype, noise_frames, with_margin      # noqa: F401 (the definitions of §6f that §6g names: coded size, element type, margin)

CLASSES = ("wt_P", "wt_N", "wt_none", "m_decides", "ws_none", "ws_full")
NEIGHBOURS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]
KERNEL = ((1, 2, 1), (2, 4, 2), (1, 2, 1))


def shifted(F, dy, dx):
    """F[y + dy][x + dx] with both indices clamped into the plane"""
    H, W = F.shape
    return F[np.clip(np.arange(H) + dy, 0, H - 1)][:, np.clip(np.arange(W) + dx, 0, W - 1)]


def filter_plane(P, C, N, depth, spatial, temporal, counts=None):
    """one plane of the display size; spatial, temporal: the plane's strengths in 8-bit units"""
    peak = (1 << depth) - 1
    P, C, N = (np.minimum(np.asarray(p).astype(np.int64), peak) for p in (P, C, N))
    assert P.shape == C.shape == N.shape and 0 <= spatial <= 255 and 0 <= temporal <= 255 and depth in (8, 10)
    counts = collections.Counter() if counts is None else counts
    Ts, Tt = spatial << (depth - 8), temporal << (depth - 8)
    wc = max(Ts, Tt, 1)
    W = np.full(C.shape, wc, np.int64)
    acc = wc * C
    ws_zero, ws_full = np.ones(C.shape, bool), np.ones(C.shape, bool)
    for dy, dx in NEIGHBOURS:
        q = shifted(C, dy, dx)
        ws = np.maximum(0, Ts - np.abs(q - C))
        W += ws
        acc += ws * q
        ws_zero &= ws == 0
        ws_full &= ws == Ts
    wts = []
    for F in (P, N):
        D = np.abs(F - C)
        m = (sum(KERNEL[dy + 1][dx + 1] * shifted(D, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) + 8) >> 4
        d = np.maximum(D, m)
        wt = np.maximum(0, Tt - d)
        W += wt
        acc += wt * F
        wts.append(wt)
        counts["m_decides"] += int((m > D).sum())
    assert W.min() >= 1 and W.max() <= 11 * 1020 and (acc + W // 2).max() < 1 << 24
    out = (acc + (W >> 1)) // W
    assert out.min() >= 0 and out.max() <= peak, "the definition's result left [0, peak]"
    counts["wt_P"] += int((wts[0] > 0).sum())
    counts["wt_N"] += int((wts[1] > 0).sum())
    counts["wt_none"] += int(((wts[0] == 0) & (wts[1] == 0)).sum())
    counts["ws_none"] += int(ws_zero.sum())
    counts["ws_full"] += int(ws_full.sum())
    return out


def strengths(s):
    """a level 0 .. 3 or four thresholds -> (luma_spatial, luma_temporal, chroma_spatial, chroma_temporal)"""
    return LEVELS[s] if isinstance(s, int) else tuple(s)


LEVELS = ((0, 0, 0, 0), (3, 4, 3, 4), (5, 7, 5, 7), (8, 11, 8, 11))


def denoise(prev, cur, nxt, depth, strength):
    """prev / cur / nxt: (Y, Cb, Cr) of three frames, display size W x H (both even and >= 16).  -> ([Y, Cb, Cr] of the coded size, [Counter per plane])"""
    H, W = cur[0].shape
    assert W >= 16 and H >= 16 and W % 2 == 0 and H % 2 == 0
    ls, lt, cs, ct = strengths(strength)
    pw, ph = coded(W), coded(H)
    out, counts = [], []
    for i in range(3):
        counts.append(collections.Counter())
        o = filter_plane(prev[i], cur[i], nxt[i], depth, cs if i else ls, ct if i else lt, counts[-1])
        out.append(np.ascontiguousarray(with_margin(o, pw if i == 0 else pw // 2, ph if i == 0 else ph // 2).astype(dtype(depth))))
    return out, counts


def pictures(frames, depth, strength):
    """the sequence rules of a session: [(pts, [Y, Cb, Cr] of the coded size)] for frames sent with pts = i; strength: one for all, or a list with one per frame"""
    per = strength if isinstance(strength, list) else [strength] * len(frames)
    return [(i, denoise(frames[max(i - 1, 0)], cur, frames[min(i + 1, len(frames) - 1)], depth, per[i])[0]) for i, cur in enumerate(frames)]


# ------------------------------------------------------------------------------------------------ inputs of the tests
def clean_frames(w, h, depth, n, speed, seed=0, clipped=True):
    """n frames of a sinusoid with a hard-edged checker on top, moving `speed` samples per frame to the right; no noise.  The pattern overshoots black and white
    by 4 % of the range, so a picture has flat areas at both ends of it, where the noise is clipped away; clipped: to [0, peak], what a picture can hold"""
    peak = (1 << depth) - 1
    frames = []
    for t in range(n):
        planes = []
        for k, (hh, ww) in enumerate(((h, w), (h // 2, w // 2), (h // 2, w // 2))):
            yy, xx = np.mgrid[0:hh, 0:ww]
            x = xx - speed * t / (2 if k else 1)
            v = 0.5 + 0.3 * np.sin(x / (25.0 - 12 * (k > 0)) + yy / 31.0) + 0.25 * np.sign(np.sin(x / 9.0) * np.sin(yy / 7.0 + seed))
            planes.append(np.clip(v * peak, 0, peak) if clipped else v * peak)
        frames.append(tuple(planes))
    return frames


def noisy_frames(w, h, depth, n, speed, sigma=2.0, seed=0):
    """(noisy frames in the depth's element type, the clean frames as floats): Gaussian noise of `sigma` LSB of 8 bit on top of clean_frames"""
    peak = (1 << depth) - 1
    rng = np.random.default_rng(1000 + seed)
    clean = clean_frames(w, h, depth, n, speed, seed, clipped=False)
    noisy = [tuple(np.ascontiguousarray(np.clip(np.rint(p + rng.normal(0, sigma * (1 << (depth - 8)), p.shape)), 0, peak).astype(dtype(depth))) for p in f) for f in clean]
    return noisy, [tuple(np.clip(p, 0, peak) for p in f) for f in clean]


def psnr(a, b, depth):
    peak = (1 << depth) - 1
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return 10 * np.log10(peak * peak / mse) if mse else float("inf")
