"""Sign data hiding (mihevc_config.sign_hide, H.265 7.3.8.11 / 9.3.4.3): the parity rule the kernels apply to every 4x4 coefficient group, in plain Python on
numpy arrays, as DESIGN.md §3 states it.  tests/test_sign_hiding_cpu.py holds the stepped kernels' K3 to it; tests/hevc_inter_cu.py applies it to the inter TUs.

Imports: numpy and the standard library only (tests/test_syntax_independent.py checks it)."""
import numpy as np  # noqa: F401  (lv and c are numpy arrays)


def scan4(scan):
    """raster positions (y * 4 + x) of scan positions 0..15 of a 4x4 group: 6.5.3 up-right diagonal, 6.5.4 horizontal, 6.5.5 vertical"""
    if scan == 1:
        return [y * 4 + x for y in range(4) for x in range(4)]
    if scan == 2:
        return [y * 4 + x for x in range(4) for y in range(4)]
    out, x, y = [], 0, 0
    while len(out) < 16:
        while y >= 0:
            if x < 4 and y < 4:
                out.append(y * 4 + x)
            y, x = y - 1, x + 1
        y, x = x, 0
    return out


def scan_idx(log2n, c_idx, mode):
    """7.4.9.11"""
    if log2n == 2 or (log2n == 3 and c_idx == 0):
        if 6 <= mode <= 14:
            return 2
        if 22 <= mode <= 30:
            return 1
    return 0


def hide_group(lv, c, scan, qs, qbits):
    """the parity adjustment of one 4x4 group (lv, c: 4x4 levels and forward coefficients; lv is changed in place), as the issue states it"""
    order = scan4(scan)
    L = [int(lv[p // 4, p % 4]) for p in order]
    cf = [int(c[p // 4, p % 4]) for p in order]
    nz = [n for n in range(16) if L[n]]
    if not nz or nz[-1] - nz[0] <= 3:
        return
    first, last = nz[0], nz[-1]
    sf = int(L[first] < 0)
    if sum(abs(v) for v in L) & 1 == sf:
        return
    best = None
    for n in range(last, -1, -1):
        a, u = abs(L[n]), abs(cf[n]) * qs
        delta = (u - (a << qbits)) >> (qbits - 8)
        if a:
            if delta > 0:
                chg, cost = 1, -delta
            elif n == first and a == 1:
                continue
            else:
                chg, cost = -1, delta
        else:
            if n < first and int(cf[n] < 0) != sf:
                continue
            chg, cost = 1, -delta
        if best is None or cost < best[0]:
            best = (cost, n, chg)
    _, n, chg = best
    a = abs(L[n])
    if chg == 1 and a == 32767:
        chg = -1
    a += chg
    p = order[n]
    lv[p // 4, p % 4] = a if cf[n] >= 0 else -a
