"""NumPy float64 restatement of scipy.signal.resample_poly, written from its documented behaviour and independent of
the package: the taps times up, the row extended by the pad type, and

    y[n] = bg + Σ_m h[half_len + n·down − m·up] · ext(x − bg, m)     over the m that keep the tap index in range,

0 <= n < ceil(T up / down).  Shared by test_resample_cpu.py and test_resample_gpu.py, with the shapes and the data.

No test may hand scipy a one-sample row with 'edge', 'reflect', 'symmetric', 'line' or 'wrap': scipy 1.15.3 dies with a
floating point exception there."""
import math

import numpy as np
from scipy.signal import firwin

RATIOS = [(1, 2), (1, 4), (2, 1), (7, 1), (3, 2), (2, 3), (125, 512), (160, 147), (4, 16)]
PADTYPES = ["constant", "edge", "reflect", "symmetric", "line", "mean", "median", "minimum", "maximum"]
STATS = {"mean": np.mean, "median": np.median, "minimum": np.amin, "maximum": np.amax}
TAPS = {n: np.random.default_rng(100 + n).standard_normal(n) for n in (1, 2, 31, 32)}      # explicit windows


def design(up, down, window=("kaiser", 5.0)):
    """-> (up, down, h, half_len): up / down reduced, h already times up."""
    g = math.gcd(up, down)
    up, down = up // g, down // g
    if isinstance(window, (list, np.ndarray)):
        h = np.asarray(window, dtype=np.float64)
        half_len = (h.size - 1) // 2
    else:
        max_rate = max(up, down)
        half_len = 10 * max_rate
        h = firwin(2 * half_len + 1, 1.0 / max_rate, window=window)
    return up, down, h * up, half_len


def ext(x, m, mode, cval):
    """Samples ``m`` (int array) of the rows ``x`` [R, T] extended by ``mode`` -> [R, len(m)]."""
    T = x.shape[-1]
    inside = (m >= 0) & (m < T)
    if mode == "constant":
        out = np.full(x.shape[:-1] + m.shape, float(cval))
        out[..., inside] = x[..., m[inside]]
        return out
    if mode == "edge":
        return x[..., np.clip(m, 0, T - 1)]
    if mode == "reflect":
        p = 2 * (T - 1)
        r = m % p
        return x[..., np.where(r < T, r, p - r)]
    if mode == "symmetric":
        p = 2 * T
        r = m % p
        return x[..., np.where(r < T, r, p - 1 - r)]
    if mode == "line":
        line = x[..., :1] + (x[..., -1:] - x[..., :1]) / (T - 1) * m
        line[..., inside] = x[..., m[inside]]
        return line
    raise ValueError(mode)


def resample_poly(x, up, down, window=("kaiser", 5.0), padtype="constant", cval=None):
    """x [..., T] -> float64 [..., ceil(T up / down)]; ``cval=None`` is 0."""
    x = np.asarray(x, dtype=np.float64)
    if up == down:
        return x.copy()
    up, down, h, half_len = design(up, down, window)
    T = x.shape[-1]
    n_out = -(-T * up // down)
    bg = 0.0
    mode = padtype
    if padtype in STATS:
        bg = STATS[padtype](x, axis=-1, keepdims=True)
        mode, cval = "constant", 0.0
    xc = x - bg
    y = np.zeros(x.shape[:-1] + (n_out,))
    L = h.size
    for n in range(n_out):
        c = half_len + n * down
        m = np.arange(-((L - 1 - c) // up), c // up + 1)               # ceil((c − (L − 1)) / up) .. floor(c / up)
        y[..., n] = ext(xc, m, mode, 0.0 if cval is None else cval) @ h[c - m * up]
    return y + bg


def make_rows(rows, T, seed=0):
    """standard_normal + a slow sine + a per-row offset cycling through 0, 50, −200 (float64 [rows, T])."""
    rng = np.random.default_rng(seed + 1000 * rows + T)
    x = rng.standard_normal((rows, T)) + 2.0 * np.sin(2.0 * np.pi * np.arange(T) / 25.0)
    return x + np.array([0.0, 50.0, -200.0])[np.arange(rows) % 3][:, None]


def rel_err(got, ref):
    """max|got − ref| / max|ref|"""
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref)) / np.max(np.abs(ref)))
