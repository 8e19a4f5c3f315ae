"""The deinterlacer of DESIGN.md §6f (mihevc_send_frame_deint / mihevc_k_deinterlace) as a numpy model, written from the definition and not from the kernel: no
tiles, no runs, no staging; whole planes of Python ints (int64), one statement per line of the definition.  deinterlace() returns the three planes of the CODED
size and a Counter of the branches taken; the sequence rules of a session are in pictures()."""
import collections

import numpy as np


def coded(n):
    return (n + 7) & ~7


def dtype(depth):
    return np.uint8 if depth == 8 else np.dtype("<u2")


def _rows(plane, rows):
    """plane[r] for the row indices `rows`, a row below 0 replaced by r + 2 and one past the last by r - 2"""
    H = plane.shape[0]
    r = np.where(rows < 0, rows + 2, np.where(rows >= H, rows - 2, rows))
    assert r.min() >= 0 and r.max() < H
    return plane[r]


def _cols(rows, off):
    """rows[:, x + off] with the column index clamped into the plane"""
    W = rows.shape[1]
    return rows[:, np.clip(np.arange(W) + off, 0, W - 1)]


def filter_plane(P, C, N, depth, keep, second, counts=None):
    """one plane W x H (display size): the kept rows of C and the interpolated rows between them"""
    peak = (1 << depth) - 1
    P, C, N = (np.minimum(np.asarray(p).astype(np.int64), peak) for p in (P, C, N))
    H, W = C.shape
    assert H >= 4 and H % 2 == 0 and P.shape == C.shape == N.shape and keep in (0, 1) and second in (0, 1)
    counts = collections.Counter() if counts is None else counts
    out = C.copy()
    ys = np.arange(1 - keep, H, 2)                     # the missing rows
    A, Z = (C, N) if second else (P, C)
    c, e = _rows(C, ys - 1), _rows(C, ys + 1)
    d = (A[ys] + Z[ys]) >> 1
    t0 = np.abs(A[ys] - Z[ys])
    t1 = (np.abs(_rows(P, ys - 1) - c) + np.abs(_rows(P, ys + 1) - e)) >> 1
    t2 = (np.abs(_rows(N, ys - 1) - c) + np.abs(_rows(N, ys + 1) - e)) >> 1
    diff = np.maximum(np.maximum(t0 >> 1, t1), t2)
    first = np.where((t0 >> 1) == diff, 0, np.where(t1 == diff, 1, 2))       # which term set diff (the first of equals)

    def score(j):
        return sum(np.abs(_cols(c, k + j) - _cols(e, k - j)) for k in (-1, 0, 1))

    def pred(j):
        return (_cols(c, j) + _cols(e, -j)) >> 1

    best, sp = score(0) - 1, pred(0)
    won = np.zeros_like(sp)
    for s in (-1, 1):
        one = score(s) < best
        best, sp, won = np.where(one, score(s), best), np.where(one, pred(s), sp), np.where(one, s, won)
        two = one & (score(2 * s) < best)              # tried only where s itself won
        best, sp, won = np.where(two, score(2 * s), best), np.where(two, pred(2 * s), sp), np.where(two, 2 * s, won)
    b = (_rows(A, ys - 2) + _rows(Z, ys - 2)) >> 1
    f = (_rows(A, ys + 2) + _rows(Z, ys + 2)) >> 1
    mx = np.maximum(np.maximum(d - e, d - c), np.minimum(b - c, f - e))
    mn = np.minimum(np.minimum(d - e, d - c), np.maximum(b - c, f - e))
    wide = np.maximum(np.maximum(diff, mn), -mx)
    res = np.where(sp > d + wide, d + wide, np.where(sp < d - wide, d - wide, sp))
    assert res.min() >= 0 and res.max() <= peak, "the definition's result left [0, peak]"
    out[ys] = res
    for j in (-2, -1, 0, 1, 2):
        counts[f"offset{j:+d}"] += int((won == j).sum())
    counts["clamp_high"] += int((sp > d + wide).sum())
    counts["clamp_low"] += int((sp < d - wide).sum())
    counts["clamp_none"] += int(((sp <= d + wide) & (sp >= d - wide)).sum())
    for k, name in enumerate(("diff_t0", "diff_t1", "diff_t2")):
        counts[name] += int((first == k).sum())
    counts["widened"] += int((wide > diff).sum())
    return out


BRANCHES = [f"offset{j:+d}" for j in (-2, -1, 0, 1, 2)] + ["clamp_high", "clamp_low", "clamp_none", "diff_t0", "diff_t1", "diff_t2", "widened"]


def with_margin(plane, pw, ph):
    """output sample (x, y) outside the display area equals the one at (min(x, W - 1), min(y, H - 1))"""
    H, W = plane.shape
    return plane[np.minimum(np.arange(ph), H - 1)][:, np.minimum(np.arange(pw), W - 1)]


def deinterlace(prev, cur, nxt, depth, keep, second):
    """prev / cur / nxt: (Y, Cb, Cr) of three frames, display size W x H (W even, H a multiple of 4, both >= 16).  -> ([Y, Cb, Cr] of the coded size, Counter)"""
    H, W = cur[0].shape
    assert W >= 16 and H >= 16 and W % 2 == 0 and H % 4 == 0
    counts = collections.Counter()
    pw, ph = coded(W), coded(H)
    out = []
    for i in range(3):
        o = filter_plane(prev[i], cur[i], nxt[i], depth, keep, second, counts)
        out.append(np.ascontiguousarray(with_margin(o, pw if i == 0 else pw // 2, ph if i == 0 else ph // 2).astype(dtype(depth))))
    return out, counts


def pictures(frames, depth, tff=True, field_rate=False):
    """the sequence rules of a session: [(pts, [Y, Cb, Cr] of the coded size)] for frames sent with pts = i (frame rate) or 2 i (field rate)"""
    out = []
    first = 0 if tff else 1
    for i, cur in enumerate(frames):
        prev, nxt = frames[max(i - 1, 0)], frames[min(i + 1, len(frames) - 1)]
        if not field_rate:
            out.append((i, deinterlace(prev, cur, nxt, depth, first, 0)[0]))
        else:
            out.append((2 * i, deinterlace(prev, cur, nxt, depth, first, 0)[0]))
            out.append((2 * i + 1, deinterlace(prev, cur, nxt, depth, 1 - first, 1)[0]))
    return out


# ------------------------------------------------------------------------------------------------ inputs of the tests
def noise_frames(w, h, depth, seed, full_word=True):
    """three frames of full-range noise; at 10 bit with values above the depth too (full_word), which the definition clamps"""
    rng = np.random.default_rng(seed)
    top = 65536 if depth > 8 and full_word else (1 << depth)
    def plane(hh, ww):
        p = rng.integers(0, top, (hh, ww))
        if depth > 8 and full_word:      # most samples inside the depth, some far above it
            p = np.where(rng.random((hh, ww)) < 0.9, p & 1023, p)
        return np.ascontiguousarray(p.astype(dtype(depth)))
    return [(plane(h, w), plane(h // 2, w // 2), plane(h // 2, w // 2)) for _ in range(3)]


def woven_frames(w, h, depth, n, tff=True, seed=0):
    """n woven frames of a moving sinusoid with an oblique edge: field 2 i comes from time 2 i, field 2 i + 1 from time 2 i + 1, the first field in time on the
    rows of parity 0 (tff) or 1"""
    peak = (1 << depth) - 1
    rng = np.random.default_rng(seed)

    def progressive(t, hh, ww, k):
        yy, xx = np.mgrid[0:hh, 0:ww]
        v = 0.5 + 0.3 * np.sin((xx + 3 * t) / (5.0 + k) + yy / 9.0) + 0.2 * np.sign(np.sin((xx - yy + 5 * t) / 17.0))
        return np.clip(np.rint(v * peak + rng.normal(0, peak / 200.0, (hh, ww))), 0, peak)

    frames = []
    for i in range(n):
        planes = []
        for k, (hh, ww) in enumerate(((h, w), (h // 2, w // 2), (h // 2, w // 2))):
            a, b = progressive(2 * i, hh, ww, k), progressive(2 * i + 1, hh, ww, k)
            f = a.copy()
            second_rows = slice(1, None, 2) if tff else slice(0, None, 2)
            f[second_rows] = b[second_rows]
            planes.append(np.ascontiguousarray(f.astype(dtype(depth))))
        frames.append(tuple(planes))
    return frames
