"""Polyphase resampling on the GPU: the change of sampling rate in front of every other step of the chain.

``resample_poly(x, up, down, ...)`` has the argument order, defaults and arithmetic of ``scipy.signal.resample_poly``:
the row is extended by ``padtype``, raised by ``up`` with zeros, low-pass filtered by a zero-phase FIR and every
``down``-th sample kept, ``ceil(T up / down)`` of them,

    y[n] = Σ_m xe[m] · h[half_len + n·down − m·up]      over the m with 0 ≤ half_len + n·down − m·up < len(h),

where ``h`` is ``up · firwin(2·half_len + 1, 1 / max(up, down), window=window)`` with ``half_len = 10 max(up, down)``,
or the taps handed over as ``window`` times ``up``.  A 1024 Hz recording becomes a 256 Hz one with
``resample_poly(X, 1, 4)`` and a 250 Hz one with ``resample_poly(X, 125, 512)`` without leaving the card.

``resample(x, up, down, ...)`` has the surface of ``mne.filter.resample`` for ``method='polyphase'``.  MNE is not
vendored in the reference and is not installed here: its surface is restated from its documentation, and parity with
MNE -- its output length rule included -- is not pinned.  MNE's default is ``method='fft'``, which is not provided.

The taps and every argument check are host work (``resample_design``, NumPy and ``scipy.signal.firwin``); the product
runs in libisd_hip.so (csrc/resample.hip) on the fp32 / fp64 matrix cores.  There is no CPU fallback.  Not provided:
an FFT resampler, a gradient, bf16, and scipy's pad types 'wrap', 'smooth', 'antireflect' and 'antisymmetric'.
"""
import fractions
import functools
import math
import operator
from collections import namedtuple

import numpy as np
import torch

from . import _lib

MAX_RATE = 1024                      # isd_resample_plan_create: reduced up, down <= 1024
MAX_TAPS = 20 * MAX_RATE + 1         # ... and at most the taps of the automatic design at that rate

ResampleDesign = namedtuple("ResampleDesign", "up down taps half_len")

_MODES = {"constant": 0, "edge": 1, "reflect": 2, "symmetric": 3, "line": 4}      # ISD_RESAMPLE_*
_STAT_PADS = ("mean", "median", "minimum", "maximum")
_NOT_PROVIDED_PADS = ("wrap", "smooth", "antireflect", "antisymmetric")
PADTYPES = tuple(_MODES) + _STAT_PADS


def _rates(up, down):
    try:
        up_i, down_i = operator.index(up), operator.index(down)
    except TypeError:
        if not (float(up).is_integer() and float(down).is_integer()):
            raise ValueError(f"up={up!r} and down={down!r} must be integers") from None
        up_i, down_i = int(up), int(down)
    if up_i < 1 or down_i < 1:
        raise ValueError(f"up={up!r} and down={down!r} must be >= 1")
    g = math.gcd(up_i, down_i)
    return up_i // g, down_i // g


def out_len(T, up, down):
    """Samples ``resample_poly`` returns for a row of T: ceil(T up / down) with up / down reduced."""
    up, down = _rates(up, down)
    return -(-int(T) * up // down)


def resample_design(up, down, window=("kaiser", 5.0)):
    """Resolve ``up``, ``down`` and ``window`` as ``scipy.signal.resample_poly`` does; never touches the GPU.

    -> ResampleDesign(up, down, taps, half_len): up / down reduced by their gcd; ``taps`` (float64) already times
    ``up``; ``half_len`` the index of the tap that meets the output's own instant.  A list or ndarray ``window`` is
    the taps as given (any length >= 1, ``half_len = (size − 1) // 2``); anything else is handed to
    ``scipy.signal.firwin(2·half_len + 1, 1 / max(up, down), window=window)`` with ``half_len = 10 max(up, down)``
    (``up == down`` has no such filter -- scipy returns a copy -- and gets the single tap 1)."""
    up, down = _rates(up, down)
    if isinstance(window, (list, np.ndarray)):
        h = np.array(window, dtype=np.float64)
        if h.ndim != 1 or h.size < 1:
            raise ValueError(f"window must be a one-dimensional array of taps, got shape {h.shape}")
        if not np.all(np.isfinite(h)):
            raise ValueError("window taps must be finite")
        half_len = (h.size - 1) // 2
    elif up == down:                                               # scipy copies before it designs: the identity
        h, half_len = np.ones(1), 0
    else:
        from scipy.signal import firwin
        max_rate = max(up, down)
        half_len = 10 * max_rate
        h = firwin(2 * half_len + 1, 1.0 / max_rate, window=window)
    return ResampleDesign(up, down, np.ascontiguousarray(h * up), half_len)


def phase_tables_shape(d):
    """(number of phase tables, samples K of a block's window) of the plan csrc/resample.hip builds for a design: a
    block of 16 outputs starting at phase phi = 16 b down mod up reads the samples c(phi) .. last(phi) past its
    origin; K is the longest such window rounded up to 4."""
    step = math.gcd(d.up, 16 * d.down)
    L, K = d.taps.size, 0
    for phi in range(0, d.up, step):
        c0 = -((L - 1 - d.half_len - phi) // d.up)
        K = max(K, (d.half_len + phi + 15 * d.down) // d.up - c0 + 1)
    return d.up // step, (K + 3) // 4 * 4


def _check_envelope(d):
    if d.up > MAX_RATE or d.down > MAX_RATE:
        raise NotImplementedError(f"up / down = {d.up} / {d.down} after reduction: at most {MAX_RATE} is provided")
    if d.taps.size > MAX_TAPS:
        raise NotImplementedError(f"{d.taps.size} taps: at most {MAX_TAPS} are provided")


class Resampler(_lib.Handle):
    """Plan for one (up, down, window) on the current device: host taps (float64) + the phase tables of
    csrc/resample.hip.  ``up == down`` after reduction needs no plan and copies."""
    _destroy = "isd_resample_plan_destroy"

    def __init__(self, up, down, window=("kaiser", 5.0)):
        d = resample_design(up, down, window)
        self.up, self.down, self.taps, self.half_len = d
        self._h = None
        if (self.up, self.down) != (1, 1):
            _check_envelope(d)
            try:
                self._create("isd_resample_plan_create", self.up, self.down, int(self.taps.size),
                             _lib.double_array(self.taps), int(self.half_len))
            except _lib.IsdUnsupported as e:
                raise NotImplementedError(str(e)) from None

    def out_len(self, T):
        return -(-int(T) * self.up // self.down)

    def __call__(self, x, padtype="constant", cval=None, out=None):
        """x CUDA tensor [..., T], float32 (fp32 arithmetic) or float64 (fp64 arithmetic) -> [..., n_out], same dtype."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype in (torch.float32, torch.float64)):
            raise TypeError("x must be a float32 or float64 CUDA tensor")
        mode, cval, stat = _resolve_pad(padtype, cval)
        if x.ndim < 1:
            raise ValueError("x must have a time axis")
        x = x.contiguous()
        T = int(x.shape[-1])
        _check_length(T, padtype)
        n_out = self.out_len(T)
        if n_out >= 2 ** 31:
            raise NotImplementedError(f"{n_out} output samples per row: fewer than 2^31 are provided")
        shape = tuple(x.shape[:-1]) + (n_out,)
        rows = x.numel() // T
        if out is None:
            out = torch.empty(shape, dtype=x.dtype, device=x.device)
        elif (tuple(out.shape) != shape or out.dtype != x.dtype or out.device != x.device
              or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous {x.dtype} tensor of shape {shape} on x's device")
        if rows and out.data_ptr() == x.data_ptr():
            raise ValueError("in-place resampling is not supported")
        if rows == 0:
            return out
        if self._h is None:                                        # up == down: a copy
            return out.copy_(x)
        x2 = x.reshape(rows, T)
        with torch.cuda.device(x.device):
            bg = _background(x2, stat)
            fn = _lib.typed("isd_resample_poly", x.dtype)
            try:
                _lib.check(fn(self._h, x2.data_ptr(), out.data_ptr(), rows, T, mode, cval,
                              bg.data_ptr() if bg is not None else None, _lib.stream()))
            except _lib.IsdUnsupported as e:
                raise NotImplementedError(str(e)) from None
        return out


def _check_length(T, padtype):
    if T < 1:
        raise ValueError("x has no samples along the time axis")
    if T < 2 and padtype in ("reflect", "line"):
        raise ValueError(f"padtype={padtype!r} needs at least two samples per row")


def _resolve_pad(padtype, cval):
    """-> (library mode, cval, statistic or None); scipy's own errors for a cval without 'constant'."""
    if padtype in _NOT_PROVIDED_PADS:
        raise NotImplementedError(f"padtype={padtype!r} is not provided: one of {PADTYPES}")
    if padtype not in PADTYPES:
        raise ValueError(f"padtype={padtype!r}: need one of {PADTYPES}")
    if cval is not None and padtype != "constant":
        raise ValueError("cval has no effect unless padtype is 'constant'")
    if padtype in _STAT_PADS:
        return _MODES["constant"], 0.0, padtype
    return _MODES[padtype], float(cval) if cval is not None else 0.0, None


def _background(x2, stat):
    """The row statistic of a statistic pad type as fp64 [rows] on x's device (None without one)."""
    if stat is None:
        return None
    if stat == "mean":
        bg = x2.mean(dim=-1, dtype=torch.float64)
    elif stat == "minimum":
        bg = x2.amin(dim=-1)
    elif stat == "maximum":
        bg = x2.amax(dim=-1)
    else:                                                          # np.median: the two middle values averaged
        v, T = torch.sort(x2, dim=-1).values.double(), x2.shape[-1]
        bg = (v[:, (T - 1) // 2] + v[:, T // 2]) * 0.5
    return bg.to(torch.float64).contiguous()


@functools.lru_cache(maxsize=16)
def _cached_plan(up, down, window, taps_bytes, device_index):
    """Resampler by value: ``window`` what firwin takes, or None with the taps' bytes in ``taps_bytes``."""
    if taps_bytes is not None:
        window = np.frombuffer(taps_bytes, dtype=np.float64)
    with torch.cuda.device(device_index):
        return Resampler(up, down, window)


def _window_key(window):
    if isinstance(window, (list, np.ndarray)):
        return None, np.ascontiguousarray(window, dtype=np.float64).tobytes()
    return (tuple(window) if isinstance(window, (list, tuple)) else window), None


def resample_poly(x, up, down, axis=-1, window=("kaiser", 5.0), padtype="constant", cval=None):
    """Resample ``x`` along ``axis`` by up / down -- argument order and defaults of ``scipy.signal.resample_poly``.
    ndarray in -> computed in fp64 on the GPU -> float64 ndarray out; float32 / float64 CUDA tensor in -> CUDA tensor
    of that dtype out.  ``padtype``: 'constant' (``cval``, default 0), 'edge', 'reflect', 'symmetric', 'line', 'mean',
    'median', 'minimum', 'maximum'; scipy's 'wrap', 'smooth', 'antireflect' and 'antisymmetric' raise
    NotImplementedError."""
    up_r, down_r = _rates(up, down)
    _resolve_pad(padtype, cval)
    x, is_tensor = _lib.check_array(x, "x")
    if x.ndim < 1:
        raise ValueError("x must have a time axis")
    axis = operator.index(axis)
    if not -x.ndim <= axis < x.ndim:
        raise ValueError(f"axis={axis} is out of bounds for {x.ndim} dimensions")
    _check_length(int(x.shape[axis]), padtype)
    key, taps_bytes = _window_key(window)
    if (up_r, down_r) != (1, 1):
        _check_envelope(_cached_design(up_r, down_r, key, taps_bytes))
    xd = x if is_tensor else _lib.to_device(x, False, "resample_poly")   # a tensor is made contiguous after movedim
    plan = _cached_plan(up_r, down_r, key, taps_bytes, xd.device.index)
    y = plan(xd.movedim(axis, -1).contiguous(), padtype, cval).movedim(-1, axis)
    return y if is_tensor else np.ascontiguousarray(y.cpu().numpy())


@functools.lru_cache(maxsize=64)
def _cached_design(up, down, window, taps_bytes):
    if taps_bytes is not None:
        window = np.frombuffer(taps_bytes, dtype=np.float64)
    return resample_design(up, down, window)


def resample(x, up=1.0, down=1.0, *, axis=-1, window="auto", n_jobs=None, pad="auto", npad="auto",
             method="polyphase", verbose=None):
    """Resample ``x`` along ``axis`` by up / down -- the surface of ``mne.filter.resample`` for
    ``method='polyphase'``: ``window='auto'`` is ``('kaiser', 5.0)``, ``pad='auto'`` is ``'reflect'``, and up / down
    (floats allowed, as MNE takes them) become the ratio of integers ``fractions.Fraction`` finds.  The result is
    ``resample_poly(x, p, q, axis, window, padtype=pad)`` bit for bit.  ``method='fft'`` -- MNE's default -- raises
    NotImplementedError; ``npad`` belongs to it and is ignored, as are ``n_jobs`` and ``verbose``.  MNE is not
    installed here: parity with MNE, its output length rule included, is not pinned."""
    if method != "polyphase":
        raise NotImplementedError(f"method={method!r}: only 'polyphase' is provided (MNE's default 'fft' is not)")
    if not (float(up) > 0 and float(down) > 0 and math.isfinite(float(up)) and math.isfinite(float(down))):
        raise ValueError(f"up={up!r} and down={down!r} must be positive and finite")
    ratio = (fractions.Fraction(up) / fractions.Fraction(down)).limit_denominator(10 ** 6)
    if ratio <= 0:
        raise ValueError(f"up / down = {up!r} / {down!r} is not a ratio of positive integers")
    return resample_poly(x, ratio.numerator, ratio.denominator, axis=axis,
                         window=("kaiser", 5.0) if isinstance(window, str) and window == "auto" else window,
                         padtype="reflect" if pad == "auto" else pad)
