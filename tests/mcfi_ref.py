"""The numpy model of frame-rate multiplication, written from the definition alone: tests hold the device kernels (test_gpu_mcfi.py) and the stepped
programs (test_mcfi_cpu.py) to it bit for bit.  Everything is integer; planes are numpy arrays [rows, columns]; a vector field is int16 [nby, nbx, 2] = (vx, vy)."""
import numpy as np

R1, R0, VMAX = 8, 2, 18


def dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def sample(plane, depth):
    """v = min(raw, 2^B - 1)"""
    return np.minimum(np.asarray(plane).astype(np.int64), (1 << depth) - 1)


def blocks(n):
    return (n + 7) // 8


def search_images(luma, depth):
    """s8 and its 2x2 mean h"""
    s8 = (sample(luma, depth) >> (depth - 8)).astype(np.int32)
    h = (s8[0::2, 0::2] + s8[0::2, 1::2] + s8[1::2, 0::2] + s8[1::2, 1::2] + 2) >> 2
    return s8, h


def at(img, ys, xs):
    """img at clamped rows ys and columns xs (arrays that broadcast against each other)"""
    return img[np.clip(ys, 0, img.shape[0] - 1), np.clip(xs, 0, img.shape[1] - 1)]


def block_sad(a, b, nby, nbx, step, size, origin, vx, vy):
    """per block (by, bx): the sum over the size x size window with origin (step bx + origin, step by + origin) of |a[p - v] - b[p + v]|; vx, vy: scalars or
    [nby, nbx] arrays"""
    if np.ndim(vx) == 0 and np.ndim(vy) == 0:          # one vector for all blocks: the difference image once, the windows' sums out of its running sums
        ys, xs = np.arange(origin, step * (nby - 1) + origin + size), np.arange(origin, step * (nbx - 1) + origin + size)
        d = np.abs(at(a, (ys - vy)[:, None], (xs - vx)[None, :]) - at(b, (ys + vy)[:, None], (xs + vx)[None, :]))
        c = np.pad(np.cumsum(np.cumsum(d, axis=0), axis=1), ((1, 0), (1, 0)))
        i, j = step * np.arange(nby)[:, None], step * np.arange(nbx)[None, :]
        return c[i + size, j + size] - c[i, j + size] - c[i + size, j] + c[i, j]
    ys = (step * np.arange(nby) + origin)[:, None, None, None] + np.arange(size)[None, None, :, None]
    xs = (step * np.arange(nbx) + origin)[None, :, None, None] + np.arange(size)[None, None, None, :]
    vx = np.broadcast_to(np.asarray(vx, np.int64), (nby, nbx))[:, :, None, None]
    vy = np.broadcast_to(np.asarray(vy, np.int64), (nby, nbx))[:, :, None, None]
    return np.abs(at(a, ys - vy, xs - vx) - at(b, ys + vy, xs + vx)).sum(axis=(2, 3), dtype=np.int64)


def key(cost, vx, vy, idx):
    return cost * (1 << 15) + (np.abs(vx) + np.abs(vy)) * (1 << 9) + idx


def search(cur_y, next_y, depth):
    """-> v0, SAD0 as a function of a field"""
    H, W = cur_y.shape
    nby, nbx = blocks(H), blocks(W)
    sc, hc = search_images(cur_y, depth)
    sn, hn = search_images(next_y, depth)
    best = np.full((nby, nbx), 1 << 62, np.int64)
    v1 = np.zeros((nby, nbx, 2), np.int64)
    for vy in range(-R1, R1 + 1):
        for vx in range(-R1, R1 + 1):
            sad = block_sad(hc, hn, nby, nbx, 4, 8, -2, vx, vy)
            k = key(sad + 2 * (abs(vx) + abs(vy)), vx, vy, (vy + R1) * (2 * R1 + 1) + vx + R1)
            win = k < best
            best = np.where(win, k, best)
            v1[win] = (vx, vy)

    def sad0(vx, vy):
        return block_sad(sc, sn, nby, nbx, 8, 16, -4, vx, vy)
    best = np.full((nby, nbx), 1 << 62, np.int64)
    v0 = np.zeros((nby, nbx, 2), np.int64)
    for dy in range(-R0, R0 + 1):
        for dx in range(-R0, R0 + 1):
            vx, vy = 2 * v1[..., 0] + dx, 2 * v1[..., 1] + dy
            k = key(sad0(vx, vy) + 4 * (np.abs(vx) + np.abs(vy)), vx, vy, (dy + R0) * (2 * R0 + 1) + dx + R0)
            win = k < best
            best = np.where(win, k, best)
            v0[..., 0] = np.where(win, vx, v0[..., 0])
            v0[..., 1] = np.where(win, vy, v0[..., 1])
    return v0, sad0


def smooth(v0):
    """per component the 5th of 9 over the 3x3 neighbourhood, block indices clamped"""
    p = np.pad(v0, ((1, 1), (1, 1), (0, 0)), mode="edge")
    nby, nbx = v0.shape[:2]
    nine = np.stack([p[dy:dy + nby, dx:dx + nbx] for dy in range(3) for dx in range(3)])
    return np.sort(nine, axis=0)[4]


def vectors(cur_y, next_y, depth):
    """-> v0, v (int16 [nby, nbx, 2]) and the scene sum D"""
    v0, sad0 = search(cur_y, next_y, depth)
    vm = smooth(v0)
    zero = sad0(vm[..., 0], vm[..., 1]) + 4 * (np.abs(vm[..., 0]) + np.abs(vm[..., 1])) > sad0(0, 0)
    v = np.where(zero[..., None], 0, vm)
    sc, sn = search_images(cur_y, depth)[0], search_images(next_y, depth)[0]
    return v0.astype(np.int16), v.astype(np.int16), int(np.abs(sc - sn).sum(dtype=np.int64))


def is_cut(D, scene_threshold, W, H):
    return scene_threshold > 0 and D > scene_threshold * W * H


def render_plane(C, N, v, f, j, chroma):
    """one plane of picture j of f, display size.  C, N: clamped samples (int64); v: the field the picture is rendered with"""
    H, W = C.shape
    nby, nbx = v.shape[:2]
    bs, ps, sh = (4, 8, 3) if chroma else (8, 4, 2)
    d = 2 * v.astype(np.int64)
    q = (8 * d * j + f) // (2 * f)          # floor division
    e = 4 * d - q
    x, y = np.arange(W), np.arange(H)
    i0, j0 = (x - bs // 2) // bs, (y - bs // 2) // bs
    ax, ay = (x - bs // 2) - bs * i0, (y - bs // 2) - bs * j0

    def fetch(img, PX, PY):
        xi, yi, fx, fy = PX >> sh, PY >> sh, PX & (ps - 1), PY & (ps - 1)
        return ((ps - fx) * (ps - fy) * at(img, yi, xi) + fx * (ps - fy) * at(img, yi, xi + 1) + (ps - fx) * fy * at(img, yi + 1, xi) + fx * fy * at(img, yi + 1, xi + 1))
    num = np.zeros((H, W), np.int64)
    for dj in (0, 1):
        for di in (0, 1):
            bi, bj = np.clip(i0 + di, 0, nbx - 1)[None, :], np.clip(j0 + dj, 0, nby - 1)[:, None]
            w = (ay if dj else bs - ay)[:, None] * (ax if di else bs - ax)[None, :]
            A = fetch(C, ps * x[None, :] - q[bj, bi, 0], ps * y[:, None] - q[bj, bi, 1])
            B = fetch(N, ps * x[None, :] + e[bj, bi, 0], ps * y[:, None] + e[bj, bi, 1])
            num += w * ((f - j) * A + j * B)
    assert num.max() < 1 << 23
    return (num + 512 * f) // (1024 * f)


def margin(plane, pw, ph):
    return np.pad(plane, ((0, ph - plane.shape[0]), (0, pw - plane.shape[1])), mode="edge")


def render(cur, nxt, depth, f, j, v=None, D=0, mode=0, scene_threshold=10):
    """picture j of f between the frames cur and nxt (each (Y, Cb, Cr)) -> the three planes of the CODED size.  v: the final field (mode 0)"""
    H, W = cur[0].shape
    nby, nbx = blocks(H), blocks(W)
    if mode == 1:
        v = np.zeros((nby, nbx, 2), np.int64)
    elif is_cut(D, scene_threshold, W, H):
        v, j = np.zeros((nby, nbx, 2), np.int64), (0 if 2 * j <= f else f)
    pw, ph = (W + 7) & ~7, (H + 7) & ~7
    out = []
    for c in range(3):
        p = render_plane(sample(cur[c], depth), sample(nxt[c], depth), np.asarray(v), f, j, c > 0)
        out.append(margin(p, pw // 2 if c else pw, ph // 2 if c else ph).astype(dtype(depth)))
    return out


def interpolate(cur, nxt, depth, f, mode=0, scene_threshold=10):
    """the f pictures of frame cur whose successor is nxt"""
    v, D = None, 0
    if mode == 0:
        _, v, D = vectors(cur[0], nxt[0], depth)
    return [render(cur, nxt, depth, f, j, v, D, mode, scene_threshold) for j in range(f)]


def clip_pictures(frames, depth, f, mode=0, scene_threshold=10):
    """what a session gives for the clip: f pictures per frame but the last, which gives its own picture only: f (n - 1) + 1"""
    out = []
    for k in range(len(frames) - 1):
        out += interpolate(frames[k], frames[k + 1], depth, f, mode, scene_threshold)
    out.append(render(frames[-1], frames[-1], depth, f, 0, mode=1))
    return out
