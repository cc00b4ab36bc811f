"""Phase-amplitude coupling with circular-shift surrogates on the GPU: does the phase of a slow rhythm modulate the
amplitude of a fast one?  The cross-frequency side of the signal toolbox, next to ``psd``, ``tfr`` and
``connectivity``.

Definitions (the tests pin these).  For one row (trial, channel) cropped to T samples, phi_p[t] is the phase of phase
band p in radians in [-pi, pi], a_q[t] >= 0 the amplitude of amplitude band q, and for a circular shift 0 <= s < T the
shifted amplitude is a_q^s[t] = a_q[(t + s) mod T].  With B = ``n_bins`` the phase bin is

    b[t] = min(B - 1, max(0, floor((double(phi[t]) + pi) * c))),    c = B / (2 pi) formed once on the host as a double,

evaluated in fp64 in both precisions -- one add, one multiply, floor -- so it is bit for bit the NumPy expression
``np.floor((phi.astype(np.float64) + np.pi) * c)`` and no input can land in different bins in the kernel and in a
reference.  n_j is the number of samples in bin j; it does not depend on s.  Per (p, q, s):

    'mvl'  mean vector length (Canolty 2006):   | sum_t a^s[t] exp(i phi[t]) | / T
    'mi'   modulation index (Tort 2010):        m_j = (sum_{t: b[t] = j} a^s[t]) / n_j, 0 for an empty bin;
                                                P_j = m_j / sum_k m_k;  MI = 1 + sum_{j: P_j > 0} P_j log P_j / log B
    'hr'   heights ratio:                       (max_j m_j - min_j m_j) / max_j m_j, empty bins counting as 0

Shift 0 is the estimate; the shifts s_1..s_S are the surrogates (the time-lag and block-swap surrogates of the
literature: a single cut point is a circular shift).  From the surrogate values v(s_i): ``surr_mean`` and ``surr_std``
(population, ddof 0), accumulated in fp64; n_ge = #{i >= 1: v(s_i) >= v(0)}; p = (1 + n_ge) / (1 + S).  With S = 0 the
mean and std are NaN and p is 1.  A row whose amplitude is zero throughout gives NaN for 'mi' and 'hr' (0 / 0).

All three measures come out of one pass of one fused kernel pair (csrc/pac.hip): a prepass sorts each phase row's
samples by bin, and the main kernel walks the sorted samples once per (phase band, amplitude band) with one GPU lane
per shift.  In torch ops the surrogates are an [n C, A, S, T] gather.  There is no CPU fallback.

Caveat.  Circular-shift surrogates do not destroy coupling to a perfectly periodic phase: every shift of a periodic
modulation is again modulated at the same rhythm.  A CPU probe of an exact 6 Hz sinusoid modulating 40 Hz gave a raw
MI of 0.034 against 0.0003 to 0.002 elsewhere, but z of about 2 only.  The phase of real recordings drifts, so the
surrogates work there; judge synthetic sinusoids by the raw value.

The names follow the literature and loosely tensorpac's ``idpac`` table; tensorpac is not installed here and parity
with it is unpinned: the formulas above are what is pinned.  Importing this module touches neither the GPU nor the
library.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .analytic import hilbert_device
from .bandpass import FirFilter
from .filter_design import fir_design

METHODS = ("mvl", "mi", "hr")        # the order of the kernel's method axis
REFUSED_METHODS = {"ndpac": "normalised direct PAC", "plv": "phase-locking value", "gc": "Gaussian-copula PAC"}
NORMALIZE = (None, "zscore", "subtract", "divide", "subtract_divide")
MAX_T, MAX_BINS, MAX_SURROGATES = 4096, 64, 4095     # kPacMaxT, kPacMaxBins, kPacMaxSurr of csrc/pac.hip
PAC_CHUNK_BYTES = 1 << 30            # device bytes of one chunk of trials: stacked phases, amplitudes, temporaries

PacResult = namedtuple("PacResult", "pac surr_mean surr_std pvalues")
_PLANS = {}                          # (sfreq, lo, hi, device index) -> FirFilter


def draw_shifts(T, n_surrogates, random_state=None, min_shift=1):
    """-> np.int32 [1 + S]: a leading 0 (the estimate), then S shifts uniform on [min_shift, T - min_shift] from
    ``np.random.default_rng(random_state)``.  NumPy only."""
    T, S, min_shift = int(T), int(n_surrogates), int(min_shift)
    if S < 0:
        raise ValueError(f"n_surrogates={n_surrogates!r} must be >= 0")
    if min_shift < 1:
        raise ValueError(f"min_shift={min_shift} must be >= 1 (shift 0 is the estimate)")
    if T < 2 * min_shift:
        raise ValueError(f"T={T} leaves no shift in [{min_shift}, T - {min_shift}]")
    out = np.zeros(1 + S, dtype=np.int32)
    out[1:] = np.random.default_rng(random_state).integers(min_shift, T - min_shift + 1, size=S)
    return out


def _check_shifts(shifts, T):
    """A host shift table -> np.int32 [1 + S], checked."""
    s = np.asarray(shifts)
    if s.ndim != 1 or s.size < 1 or s.dtype.kind not in "iu":
        raise ValueError("shifts must be a 1-d integer array with a leading 0")
    if s[0] != 0 or (s < 0).any() or (s >= T).any():
        raise ValueError(f"shifts must start with 0 and lie in [0, {T})")
    if s.size - 1 > MAX_SURROGATES:
        raise NotImplementedError(f"{s.size - 1} surrogates: at most {MAX_SURROGATES} are provided")
    return np.array(s, dtype=np.int32)                               # a copy: writable, whatever was passed


def _check_bins(n_bins):
    if isinstance(n_bins, bool) or int(n_bins) != n_bins or int(n_bins) < 2:
        raise ValueError(f"n_bins={n_bins!r} must be an integer >= 2")
    if int(n_bins) > MAX_BINS:
        raise NotImplementedError(f"n_bins={n_bins}: at most {MAX_BINS} phase bins are provided")
    return int(n_bins)


def pac_launch(pha, amp, shifts, n_bins=18, surrogates_out=False):
    """One library call.  pha [..., P, T] phases and amp [..., A, T] amplitudes: contiguous CUDA tensors of the same
    leading shape, T and dtype (float32 or float64).  ``shifts``: a host integer array [1 + S] with a leading 0
    (checked here) or an int32 CUDA tensor of that layout (not read on the host: the kernel clamps it into range).
    -> [..., A, P, 3, 4]: per method of METHODS (value, surr_mean, surr_std, n_ge); with ``surrogates_out`` also
    [..., A, P, 3, S], every surrogate value."""
    for name, t in (("pha", pha), ("amp", amp)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in (torch.float32, torch.float64)):
            raise TypeError(f"{name} must be a float32 or float64 CUDA tensor")
        if t.ndim < 2 or not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous with at least two axes, got {tuple(t.shape)}")
    if pha.dtype != amp.dtype or pha.device != amp.device or pha.shape[:-2] != amp.shape[:-2] \
            or pha.shape[-1] != amp.shape[-1]:
        raise ValueError(f"pha {tuple(pha.shape)} {pha.dtype} and amp {tuple(amp.shape)} {amp.dtype} must share "
                         "the leading shape, T, dtype and device")
    n_bins = _check_bins(n_bins)
    lead = tuple(pha.shape[:-2])
    P, A, T = int(pha.shape[-2]), int(amp.shape[-2]), int(pha.shape[-1])
    if P < 1 or A < 1 or T < 1:
        raise ValueError(f"P={P}, A={A} and T={T} must be at least 1")
    if T > MAX_T:
        raise NotImplementedError(f"T={T} samples: at most {MAX_T} are provided")
    if isinstance(shifts, torch.Tensor):
        if not (shifts.is_cuda and shifts.dtype == torch.int32 and shifts.ndim == 1 and shifts.numel() >= 1
                and shifts.device == pha.device):
            raise TypeError("a tensor of shifts must be a 1-d int32 CUDA tensor on the data's device")
        if shifts.numel() - 1 > MAX_SURROGATES:
            raise NotImplementedError(f"{shifts.numel() - 1} surrogates: at most {MAX_SURROGATES} are provided")
        sd = shifts.contiguous()
    else:
        sd = torch.from_numpy(_check_shifts(shifts, T)).to(pha.device)
    S = int(sd.numel()) - 1
    rows = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if rows * A * P >= 2 ** 31:
        raise NotImplementedError(f"rows * A * P = {rows} * {A} * {P}: fewer than 2^31 are provided")
    out = torch.empty(lead + (A, P, 3, 4), dtype=pha.dtype, device=pha.device)
    surr = torch.empty(lead + (A, P, 3, S), dtype=pha.dtype, device=pha.device) if surrogates_out else None
    if rows:
        L = _lib.lib()
        f64 = pha.dtype == torch.float64
        work = _lib.workspace(L.isd_pac_work_bytes(rows, P, A, T, int(f64)), pha.device)
        with torch.cuda.device(pha.device):
            fn = _lib.typed("isd_pac", pha.dtype)
            _lib.check(fn(pha.data_ptr(), amp.data_ptr(), sd.data_ptr(), out.data_ptr(),
                          surr.data_ptr() if surrogates_out and S else None, rows, P, A, T, S, n_bins,
                          n_bins / (2.0 * np.pi), work.data_ptr(), _lib.stream()))
    return (out, surr) if surrogates_out else out


def _check_bands(bands, name, sfreq):
    try:
        bands = [(float(lo), float(hi)) for lo, hi in bands]
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a list of (lo, hi) pairs in Hz") from None
    if not bands:
        raise ValueError(f"{name} is empty: at least one (lo, hi) band is needed")
    for lo, hi in bands:
        if not 0.0 < lo < hi < sfreq / 2.0:
            raise ValueError(f"{name} band ({lo}, {hi}) Hz must satisfy 0 < lo < hi < sfreq / 2 = {sfreq / 2.0}")
    return bands


def _plan(sfreq, band, taps, device):
    key = (float(sfreq), band[0], band[1], device.index)
    if key not in _PLANS:
        with torch.cuda.device(device):
            _PLANS[key] = FirFilter(sfreq, band[0], band[1], taps=taps)
    return _PLANS[key]


def trial_bytes(C, P, A, Tc, n_fft, itemsize):
    """Device bytes one trial of C channels needs in ``phase_amplitude_coupling``: the stacked phases and amplitudes,
    the kernel's workspace (the sorted (cos, sin, t) records of the phases) and, per band in turn, the filtered
    signal, its spectrum, the weighted spectrum, the analytic signal and the angle or modulus (8 real arrays of
    n_fft samples)."""
    return C * ((P + A) * Tc * itemsize + P * Tc * (2 * itemsize + 4) + 8 * n_fft * itemsize)


def _normalized(v, mean, std, normalize):
    if normalize is None:
        return v
    if normalize == "zscore":
        return (v - mean) / std
    if normalize == "subtract":
        return v - mean
    if normalize == "divide":
        return v / mean
    return (v - mean) / mean                                        # 'subtract_divide'


def phase_amplitude_coupling(x, sfreq, f_pha, f_amp, method="mi", n_bins=18, n_surrogates=0, normalize=None, edges=0,
                             shifts=None, random_state=None, return_stats=False, n_fft=None, surrogate="shift"):
    """Phase-amplitude coupling of x [n, C, T] ([C, T] is n = 1) -> [n, C, A, P], real, of the input's dtype; the
    formulas and the caveat on periodic phases are in the module's docstring.

    ``f_pha`` and ``f_amp`` are lists of (lo, hi) in Hz.  Per band: ``FirFilter(sfreq, lo, hi)`` (zero phase; one
    cached plan per band and device), ``hilbert(., n_fft or T)[..., :T]``, ``angle`` for a phase band and ``abs`` for
    an amplitude band, ``edges`` samples cropped from each end (T' = T - 2 edges <= 4096), then one fused kernel pass.
    Trials run in chunks of at most ``PAC_CHUNK_BYTES`` of device memory.

    ``method`` is 'mvl', 'mi' or 'hr', or a list of them (a list returns a list; all methods share one pass).
    ``n_surrogates`` circular shifts of the amplitude are drawn by ``draw_shifts(T', n_surrogates, random_state)``,
    or ``shifts`` gives the table itself (integers, a leading 0, each in [0, T')).  ``normalize`` is None, 'zscore'
    ((v - mean) / std), 'subtract' (v - mean), 'divide' (v / mean) or 'subtract_divide' ((v - mean) / mean) with the
    surrogate mean and std, in elementwise torch ops; it needs surrogates (ValueError without), and a zero surrogate
    std or mean gives +-inf or NaN as IEEE has it.  ``return_stats=True`` returns the namedtuple
    ``PacResult(pac, surr_mean, surr_std, pvalues)`` with p = (1 + #{surrogates >= estimate}) / (1 + S).

    ndarray in -> the fp64 route -> float64 ndarray out; a float32 / float64 CUDA tensor in -> a CUDA tensor out.
    There is no CPU fallback, and every argument check runs before any GPU use.  Not provided (NotImplementedError):
    the methods 'ndpac', 'plv' and 'gc', ``surrogate='swap_trials'``, T' above 4096, more than 64 bins or 4095
    surrogates."""
    x, is_tensor = _lib.check_array(x, "x")
    if x.ndim not in (2, 3):
        raise ValueError(f"x must be [n, C, T] or [C, T], got {tuple(x.shape)}")
    squeeze = x.ndim == 2
    if squeeze:
        x = x[None]
    n, Cc, T = (int(v) for v in x.shape)
    if Cc < 1 or T < 1:
        raise ValueError(f"x must have at least one channel and one sample, got {tuple(x.shape)}")
    single = isinstance(method, str)
    names = [method] if single else list(method)
    if not names:
        raise ValueError("method is an empty list")
    for m in names:
        if m in REFUSED_METHODS:
            raise NotImplementedError(f"method {m!r} ({REFUSED_METHODS[m]}) is not provided; there are {METHODS}")
        if m not in METHODS:
            raise ValueError(f"unknown method {m!r}; there are {METHODS}")
    if surrogate == "swap_trials":
        raise NotImplementedError("surrogate='swap_trials' is not provided; there is 'shift' (circular time shifts)")
    if surrogate != "shift":
        raise ValueError(f"unknown surrogate {surrogate!r}; there is 'shift'")
    n_bins = _check_bins(n_bins)
    sfreq = float(sfreq)
    if not sfreq > 0:
        raise ValueError(f"sfreq={sfreq} must be positive")
    f_pha, f_amp = _check_bands(f_pha, "f_pha", sfreq), _check_bands(f_amp, "f_amp", sfreq)
    if isinstance(edges, bool) or int(edges) != edges or int(edges) < 0:
        raise ValueError(f"edges={edges!r} must be a non-negative integer")
    edges = int(edges)
    Tc = T - 2 * edges
    if Tc < 1:
        raise ValueError(f"edges={edges} leaves no sample of T={T}")
    if Tc > MAX_T:
        raise NotImplementedError(f"T' = {Tc} samples after cropping: at most {MAX_T} are provided")
    if n_fft is None:
        n_fft = T
    elif isinstance(n_fft, bool) or int(n_fft) != n_fft or int(n_fft) < T:
        raise ValueError(f"n_fft={n_fft!r} must be an integer >= T={T}")
    n_fft = int(n_fft)
    if normalize not in NORMALIZE:
        raise ValueError(f"unknown normalize {normalize!r}; there are {NORMALIZE}")
    if isinstance(n_surrogates, bool) or int(n_surrogates) != n_surrogates or int(n_surrogates) < 0:
        raise ValueError(f"n_surrogates={n_surrogates!r} must be a non-negative integer")
    if int(n_surrogates) > MAX_SURROGATES:
        raise NotImplementedError(f"{n_surrogates} surrogates: at most {MAX_SURROGATES} are provided")
    if shifts is not None:
        table = _check_shifts(shifts, Tc)
    else:
        table = draw_shifts(Tc, int(n_surrogates), random_state) if n_surrogates else np.zeros(1, dtype=np.int32)
    S = table.size - 1
    if normalize is not None and S == 0:
        raise ValueError(f"normalize={normalize!r} needs surrogates: give n_surrogates > 0 or shifts")
    P, A = len(f_pha), len(f_amp)
    if n * Cc * A * P >= 2 ** 31:
        raise NotImplementedError(f"n * C * A * P = {n * Cc * A * P}: fewer than 2^31 are provided")
    taps = [fir_design(sfreq, lo, hi) for lo, hi in f_pha + f_amp]        # on the host: a bad band fails here

    step = max(1, PAC_CHUNK_BYTES // trial_bytes(Cc, P, A, Tc, n_fft, x.element_size() if is_tensor else 8))
    blocks = []
    for s0 in range(0, n, step):
        xd = _lib.to_device(x[s0:s0 + step], is_tensor, "phase_amplitude_coupling")
        plans = [_plan(sfreq, band, tp, xd.device) for band, tp in zip(f_pha + f_amp, taps)]
        sd = torch.from_numpy(table).to(xd.device)
        nc = xd.shape[0]
        pha = torch.empty((nc, Cc, P, Tc), dtype=xd.dtype, device=xd.device)
        amp = torch.empty((nc, Cc, A, Tc), dtype=xd.dtype, device=xd.device)
        for i, flt in enumerate(plans):
            z = hilbert_device(flt(xd), n_fft)[..., edges:edges + Tc]
            if i < P:
                pha[:, :, i] = torch.angle(z)
            else:
                amp[:, :, i - P] = z.abs()
        blocks.append(pac_launch(pha, amp, sd, n_bins))
    if blocks:
        block = torch.cat(blocks) if len(blocks) > 1 else blocks[0]      # [n, C, A, P, 3, 4]
    else:
        dev = x.device if is_tensor else None
        block = torch.empty((0, Cc, A, P, 3, 4), dtype=x.dtype if is_tensor else torch.float64, device=dev)
    res = []
    for m in names:
        v, mean, std, n_ge = block[..., METHODS.index(m), :].unbind(-1)
        # a tensor divisor: the correctly rounded quotient (a Python scalar would be multiplied by as its reciprocal)
        fields = (_normalized(v, mean, std, normalize), mean, std, (1.0 + n_ge) / torch.full_like(n_ge, 1.0 + S))
        fields = fields if return_stats else fields[:1]
        if squeeze:
            fields = tuple(f[0] for f in fields)
        fields = tuple(f.contiguous() if is_tensor else f.cpu().numpy() for f in fields)
        res.append(PacResult(*fields) if return_stats else fields[0])
    return res[0] if single else res
