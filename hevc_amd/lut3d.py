"""3D colour tables for Encoder.set_lut3d / mihevc_set_lut3d: reading and writing .cube files, quantising to the uint16 entries the device
interpolates between, and a built-in HDR -> SDR table.  numpy only, host side, float64: no device bit depends on how a table is computed, only on its quantised
entries.

A table is an (n, n, n, 3) array indexed [b][g][r][c], the order of a .cube file (red varies fastest), 2 <= n <= 65; input and output run over [0, 1], on the
device 0 .. 65535."""
import math
from pathlib import Path

import numpy as np

MIN_N, MAX_N = 2, 65


def _check_n(n):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not MIN_N <= n <= MAX_N:
        raise ValueError(f"3D table size {n!r}: {MIN_N} .. {MAX_N} points per axis")
    return int(n)


def quantise(table) -> np.ndarray:
    """rint(clip(x, 0, 1) * 65535) in float64 (ties to even) as uint16.  Non-finite entries are refused"""
    t = np.asarray(table, np.float64)
    if not np.all(np.isfinite(t)):
        raise ValueError("a table entry is not finite")
    return np.rint(np.clip(t, 0.0, 1.0) * 65535.0).astype(np.uint16)


def as_uint16(table) -> np.ndarray:
    """what set_lut3d hands down: an (n, n, n, 3) uint16 array, C-contiguous; floats go through quantise, other integers must already lie in 0 .. 65535"""
    t = np.asarray(table)
    if t.ndim != 4 or t.shape[3] != 3 or not (t.shape[0] == t.shape[1] == t.shape[2]):
        raise ValueError(f"a 3D table is an (n, n, n, 3) array, not {t.shape}")
    _check_n(t.shape[0])
    if t.dtype.kind == "f":
        t = quantise(t)
    elif t.dtype.kind not in "ui" or (t.size and (int(t.min()) < 0 or int(t.max()) > 65535)):
        raise ValueError(f"table entries of type {t.dtype} outside 0 .. 65535")
    return np.ascontiguousarray(t, dtype=np.uint16)


def identity(n: int) -> np.ndarray:
    """the table that changes nothing: entry k of an axis is quantise(k / (n - 1)); exact on the device when n - 1 divides 65535 (n = 2, 4, 6, 16, 18, 52)"""
    n = _check_n(n)
    ax = np.arange(n, dtype=np.float64) / (n - 1)
    t = np.empty((n, n, n, 3), np.float64)
    t[..., 0] = ax[None, None, :]
    t[..., 1] = ax[None, :, None]
    t[..., 2] = ax[:, None, None]
    return quantise(t)


def read_cube(path) -> np.ndarray:
    """A .cube file as an (n, n, n, 3) float64 table.  Understood: LUT_3D_SIZE, TITLE, comments (#), blank lines, DOMAIN_MIN 0 0 0 and DOMAIN_MAX 1 1 1.
    ValueError: a 1D table, another domain, an unknown keyword, a size outside 2 .. 65, a wrong number of entries, a malformed or non-finite value"""
    name = Path(path).name
    n = None
    rows = []
    with open(path, "r", encoding="utf-8", errors="replace") as f:
        for no, line in enumerate(f, 1):
            s = line.strip()
            if not s or s.startswith("#"):
                continue
            key = s.split()[0]
            if key == "TITLE":
                continue
            if key == "LUT_1D_SIZE" or key == "LUT_1D_INPUT_RANGE":
                raise ValueError(f"{name}:{no}: a 1D table ({key}); only 3D tables are read")
            if key == "LUT_3D_SIZE":
                try:
                    n = int(s.split()[1])
                except (IndexError, ValueError):
                    raise ValueError(f"{name}:{no}: malformed LUT_3D_SIZE") from None
                if not MIN_N <= n <= MAX_N:
                    raise ValueError(f"{name}:{no}: LUT_3D_SIZE {n} outside {MIN_N} .. {MAX_N}")
                continue
            if key in ("DOMAIN_MIN", "DOMAIN_MAX"):
                try:
                    vals = [float(x) for x in s.split()[1:]]
                except ValueError:
                    vals = []
                if vals != ([0.0] * 3 if key == "DOMAIN_MIN" else [1.0] * 3):
                    raise ValueError(f"{name}:{no}: {s}: only the domain 0 0 0 .. 1 1 1 is read")
                continue
            if key[0].isalpha() or key[0] == "_":
                raise ValueError(f"{name}:{no}: unknown keyword {key}")
            try:
                vals = [float(x) for x in s.split()]
            except ValueError:
                raise ValueError(f"{name}:{no}: malformed entry {s!r}") from None
            if len(vals) != 3:
                raise ValueError(f"{name}:{no}: an entry has three values, not {len(vals)}")
            if not all(math.isfinite(v) for v in vals):
                raise ValueError(f"{name}:{no}: a value is not finite")
            rows.append(vals)
    if n is None:
        raise ValueError(f"{name}: no LUT_3D_SIZE")
    if len(rows) != n ** 3:
        raise ValueError(f"{name}: {len(rows)} entries, LUT_3D_SIZE {n} needs {n ** 3}")
    return np.asarray(rows, np.float64).reshape(n, n, n, 3)


def write_cube(path, table, title=None):
    """an (n, n, n, 3) table as a .cube file: uint16 entries as value / 65535 with ten decimals (quantise(read_cube(...)) gives them back), floats with 17
    significant digits"""
    t = np.asarray(table)
    if t.ndim != 4 or t.shape[3] != 3 or not (t.shape[0] == t.shape[1] == t.shape[2]):
        raise ValueError(f"a 3D table is an (n, n, n, 3) array, not {t.shape}")
    n = _check_n(t.shape[0])
    ints = t.dtype.kind in "ui"
    with open(path, "w", encoding="utf-8") as f:
        if title:
            f.write(f'TITLE "{title}"\n')
        f.write(f"LUT_3D_SIZE {n}\nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 1 1 1\n")
        for r, g, b in t.reshape(-1, 3).tolist():
            f.write(f"{r / 65535:.10f} {g / 65535:.10f} {b / 65535:.10f}\n" if ints else f"{r:.17g} {g:.17g} {b:.17g}\n")


# ------------------------------------------------------------------------------------------------ HDR -> SDR (DESIGN.md §6i states the curve and its constants)
_PQ_M1, _PQ_M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
_PQ_C1, _PQ_C2, _PQ_C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
_HLG_A = 0.17883277
_HLG_B = 1.0 - 4.0 * _HLG_A
_HLG_C = 0.5 - _HLG_A * math.log(4.0 * _HLG_A)
SDR_PEAK_NITS = 100.0
BT1886_GAMMA = 2.4


def pq_eotf(e):
    """SMPTE ST 2084: code value 0 .. 1 -> cd/m2"""
    p = np.power(np.clip(e, 0.0, 1.0), 1.0 / _PQ_M2)
    return 10000.0 * np.power(np.maximum(p - _PQ_C1, 0.0) / (_PQ_C2 - _PQ_C3 * p), 1.0 / _PQ_M1)


def pq_inverse_eotf(nits):
    y = np.power(np.clip(nits, 0.0, 10000.0) / 10000.0, _PQ_M1)
    return np.power((_PQ_C1 + _PQ_C2 * y) / (1.0 + _PQ_C3 * y), _PQ_M2)


def _primaries_matrix(xr, yr, xg, yg, xb, yb, xw=0.3127, yw=0.3290):
    """RGB -> XYZ of a set of primaries with white D65"""
    p = np.array([[xr / yr, xg / yg, xb / yb], [1.0, 1.0, 1.0], [(1 - xr - yr) / yr, (1 - xg - yg) / yg, (1 - xb - yb) / yb]])
    s = np.linalg.solve(p, np.array([xw / yw, 1.0, (1 - xw - yw) / yw]))
    return p * s


BT2020_TO_BT709 = np.linalg.solve(_primaries_matrix(0.640, 0.330, 0.300, 0.600, 0.150, 0.060), _primaries_matrix(0.708, 0.292, 0.170, 0.797, 0.131, 0.046))


def _tone_curve(nits, peak_nits):
    """BT.2390-style EETF on a luminance in cd/m2 -> SDR linear light 0 .. 1: in PQ space normalised to the source peak, the identity below the knee
    KS = 1.5 maxLum - 0.5 and a Hermite spline towards maxLum (the SDR peak) above it; input at or above the source peak gives 1"""
    top = pq_inverse_eotf(peak_nits)
    e1 = np.minimum(pq_inverse_eotf(nits) / top, 1.0)
    max_lum = float(pq_inverse_eotf(SDR_PEAK_NITS) / top)
    if max_lum >= 1.0:
        e2 = e1
    else:
        ks = 1.5 * max_lum - 0.5
        t = np.clip((e1 - ks) / (1.0 - ks), 0.0, 1.0)
        spline = (2 * t ** 3 - 3 * t ** 2 + 1) * ks + (t ** 3 - 2 * t ** 2 + t) * (1.0 - ks) + (-2 * t ** 3 + 3 * t ** 2) * max_lum
        e2 = np.where(e1 < ks, e1, spline)
    return np.minimum(pq_eotf(e2 * top) / SDR_PEAK_NITS, 1.0)


def hdr_to_sdr_function(rgb, transfer: str = "pq", peak_nits: float = 1000.0) -> np.ndarray:
    """BT.2020 R'G'B' under PQ or HLG, (..., 3) floats in [0, 1] -> BT.709 gamma R'G'B' in [0, 1], float64: EOTF to display light, the tone curve on the largest
    component with every component scaled alike (hue kept), the 2020 -> 709 primaries matrix, clip, inverse BT.1886 (L^(1/2.4))"""
    if transfer not in ("pq", "hlg"):
        raise ValueError(f"transfer {transfer!r}: 'pq' or 'hlg'")
    peak_nits = float(peak_nits)
    if not math.isfinite(peak_nits) or not SDR_PEAK_NITS <= peak_nits <= 10000.0:
        raise ValueError(f"peak_nits {peak_nits!r}: {SDR_PEAK_NITS:g} .. 10000")
    e = np.clip(np.asarray(rgb, np.float64), 0.0, 1.0)
    if transfer == "pq":
        nits = pq_eotf(e)
    else:       # BT.2100 HLG: inverse OETF to scene light, then the OOTF of a display of peak_nits
        scene = np.where(e <= 0.5, e * e / 3.0, (np.exp((e - _HLG_C) / _HLG_A) + _HLG_B) / 12.0)
        gamma = 1.2 + 0.42 * math.log10(peak_nits / 1000.0)
        ys = scene @ np.array([0.2627, 0.6780, 0.0593])
        nits = peak_nits * np.power(np.maximum(ys, 1e-300), gamma - 1.0)[..., None] * scene
    m = nits.max(axis=-1)
    scale = np.where(m > 0.0, _tone_curve(m, peak_nits) / np.maximum(m, 1e-300), 0.0)
    lin = (nits * scale[..., None]) @ BT2020_TO_BT709.T
    return np.power(np.clip(lin, 0.0, 1.0), 1.0 / BT1886_GAMMA)


def hdr_to_sdr(n: int = 65, transfer: str = "pq", peak_nits: float = 1000.0) -> np.ndarray:
    """the (n, n, n, 3) uint16 table of hdr_to_sdr_function at the grid points k / (n - 1)"""
    n = _check_n(n)
    ax = np.arange(n, dtype=np.float64) / (n - 1)
    grid = np.empty((n, n, n, 3), np.float64)
    grid[..., 0] = ax[None, None, :]
    grid[..., 1] = ax[None, :, None]
    grid[..., 2] = ax[:, None, None]
    return quantise(hdr_to_sdr_function(grid, transfer, peak_nits))
