"""Morlet time-frequency transform on the GPU: where in time a band's power moves.

``tfr_array_morlet(data, sfreq, freqs, ...)`` has the argument order and defaults of
``mne.time_frequency.tfr_array_morlet``; ``morlet`` and ``cwt`` are the two steps it is made of.  MNE is not vendored
in the reference and is not installed here: the behaviour is restated from its documentation (the wavelet formula
below, ``np.convolve(row, W, 'same')[::decim]`` for the transform) and pinned by an independent NumPy restatement
(tests/tfr_ref.py); parity with MNE itself is not pinned.  One deliberate difference: in ``output='itc'`` a sample
with ``|z| = 0`` contributes 0 to the mean, where MNE yields NaN.

The wavelets and every argument check are host work (pure NumPy, never the GPU); the transform runs in
libisd_hip.so (csrc/tfr.hip) as a complex FIR bank on the matrix cores that writes only what is asked for: the power
map or the phase without the complex one, and for the trial averages nothing per trial.  A float32 tensor is multiplied
and accumulated in fp32, with two exceptions: the phase and the inter-trial coherence (a mean of ``z / |z|``) take their
product in fp64 over the widened samples, because the phase of a weak sample does not survive fp32 (``'avg_power_itc'``
in float32 then costs both outputs).  Each row's mean is taken off before the product and its share added back
exactly, so an offset of the data costs no precision.  There is no CPU fallback.  Not provided: multitaper and Stockwell transforms, baseline rescaling, ``decim`` as a
slice, more than ``MAX_TAPS`` taps, ``MAX_FREQS`` frequencies or a ``decim`` above ``MAX_DECIM``, bf16, a gradient.
"""
import ctypes as C
import functools

import numpy as np
import torch

from . import _lib

MAX_TAPS = 4095                      # isd_tfr_plan_create: odd n_taps <= 4095
MAX_FREQS = 256
MAX_DECIM = 128
MODES = {"complex": 0, "power": 1, "avg_power": 2, "itc": 3, "avg_power_itc": 4, "phase": 5}
OUTPUTS = ("complex", "power", "phase", "avg_power", "itc", "avg_power_itc")


def _freqs_cycles(sfreq, freqs, n_cycles):
    sfreq = float(sfreq)
    if not sfreq > 0:
        raise ValueError(f"sfreq={sfreq!r} (need > 0)")
    freqs = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    if freqs.ndim != 1 or freqs.size == 0:
        raise ValueError(f"freqs must be a non-empty 1-D array, got shape {freqs.shape}")
    if not np.all(np.isfinite(freqs)) or np.any(freqs <= 0):
        raise ValueError(f"freqs must be positive, got {freqs[~(freqs > 0)].tolist()}")
    if np.any(freqs >= sfreq / 2.0):
        raise ValueError(f"freqs must lie below the Nyquist frequency {sfreq / 2.0:g} Hz, got "
                         f"{freqs[freqs >= sfreq / 2.0].tolist()}")
    n_cycles = np.asarray(n_cycles, dtype=np.float64)
    if n_cycles.ndim == 0:
        n_cycles = np.full(freqs.shape, float(n_cycles))
    elif n_cycles.shape != freqs.shape:
        raise ValueError(f"n_cycles must be a scalar or one value per frequency: shape {n_cycles.shape} for "
                         f"{freqs.size} frequencies")
    if not np.all(np.isfinite(n_cycles)) or np.any(n_cycles <= 0):
        raise ValueError(f"n_cycles must be positive, got {n_cycles[~(n_cycles > 0)].tolist()}")
    return sfreq, freqs, n_cycles


def morlet(sfreq, freqs, n_cycles=7.0, sigma=None, zero_mean=False):
    """Complex Morlet wavelets as ``mne.time_frequency.morlet`` documents them -> a list of complex128 arrays of odd
    lengths, one per frequency; ``n_cycles`` a scalar or one value per frequency.  Per f:
    sigma_t = n_cycles / (2 pi f) (or n_cycles / (2 pi sigma)), t = -5 sigma_t .. 5 sigma_t in steps of 1 / sfreq,
    W = (exp(2 pi i f t) - [zero_mean] exp(-2 (pi f sigma_t)^2)) exp(-t^2 / (2 sigma_t^2)), scaled to |W|_2 = sqrt 2."""
    sfreq, freqs, n_cycles = _freqs_cycles(sfreq, freqs, n_cycles)
    if sigma is not None and not float(sigma) > 0:
        raise ValueError(f"sigma={sigma!r} (need > 0)")
    Ws = []
    for f, nc in zip(freqs, n_cycles):
        sigma_t = nc / (2.0 * np.pi * (f if sigma is None else float(sigma)))
        t = np.arange(0.0, 5.0 * sigma_t, 1.0 / sfreq)
        t = np.r_[-t[::-1], t[1:]]
        osc = np.exp(2.0 * np.pi * 1j * f * t)
        if zero_mean:
            osc = osc - np.exp(-2.0 * (np.pi * f * sigma_t) ** 2)
        W = osc * np.exp(-t ** 2 / (2.0 * sigma_t ** 2))
        W /= np.sqrt(0.5) * np.linalg.norm(W.ravel())
        Ws.append(W)
    return Ws


@functools.lru_cache(maxsize=32)
def _cached_morlet(sfreq, freqs_bytes, n_cycles_bytes, zero_mean):
    """morlet by value -> (n_taps tuple, the taps of all wavelets as one complex128 byte string)."""
    Ws = morlet(sfreq, np.frombuffer(freqs_bytes, dtype=np.float64), np.frombuffer(n_cycles_bytes, dtype=np.float64),
                zero_mean=zero_mean)
    return tuple(len(W) for W in Ws), np.concatenate(Ws).tobytes()


def _check_decim(decim):
    if isinstance(decim, slice):
        raise NotImplementedError("decim as a slice is not provided: give an integer step")
    if isinstance(decim, bool) or not isinstance(decim, (int, np.integer)):
        raise TypeError(f"decim must be an integer, got {type(decim).__name__}")
    if decim < 1:
        raise ValueError(f"decim={decim} (need >= 1)")
    if decim > MAX_DECIM:
        raise NotImplementedError(f"decim={decim}: at most MAX_DECIM = {MAX_DECIM} is provided")
    return int(decim)


def _check_taps(n_taps, T):
    """The envelope of the library and MNE's rule that no wavelet is longer than the signal."""
    if len(n_taps) == 0:
        raise ValueError("no wavelets")
    if len(n_taps) > MAX_FREQS:
        raise NotImplementedError(f"{len(n_taps)} frequencies: at most MAX_FREQS = {MAX_FREQS} are provided")
    for j, L in enumerate(n_taps):
        if L < 1 or L % 2 == 0:
            raise ValueError(f"wavelet {j} has {L} taps (need an odd count)")
        if L > MAX_TAPS:
            raise NotImplementedError(f"wavelet {j} has {L} taps: at most MAX_TAPS = {MAX_TAPS} are provided")
    if max(n_taps) > T:
        j = int(np.argmax(n_taps))
        raise ValueError(f"wavelet {j} is longer than the signal: {n_taps[j]} taps against {T} samples "
                         "(use a longer signal or fewer cycles)")


def out_len(T, decim):
    """ceil(T / decim): the samples 0, decim, 2 decim, ... of a row of T."""
    return -(-int(T) // int(decim))


class TfrPlan(_lib.Handle):
    """The device tables of one complex FIR bank (tap vectors of odd lengths, decim) on one device."""
    _destroy = "isd_tfr_plan_destroy"

    def __init__(self, n_taps, taps, decim):
        """n_taps: F odd counts; taps: their complex128 values one after the other."""
        taps = np.ascontiguousarray(taps, dtype=np.complex128)
        self.n_freqs, self.decim = len(n_taps), int(decim)
        self._create("isd_tfr_plan_create", self.n_freqs, _lib.int_array(n_taps),
                     taps.view(np.float64).ctypes.data_as(C.POINTER(C.c_double)), self.decim)
        self.useful_taps = int(sum(n_taps))
        self.padded_taps = int(_lib.lib().isd_tfr_plan_padded_taps(self._h))

    def __call__(self, x, mode, out=None):
        """x contiguous CUDA [n, C, T] (f32 / f64), mode a key of MODES -> [n, C, F, T_out] (complex for 'complex')
        or, for the averaged modes, [C, F, T_out] (complex (avg_power, itc) for 'avg_power_itc').  ``out``: a
        contiguous tensor of that shape and dtype to write into."""
        L = _lib.lib()
        n, Cn, T = x.shape
        m = MODES[mode]
        f64 = x.dtype == torch.float64
        T_out = int(L.isd_tfr_plan_out_len(self._h, T))
        avg = 2 <= m <= 4
        shape = ((Cn,) if avg else (n, Cn)) + (self.n_freqs, T_out)
        dtype = x.dtype if m not in (0, 4) else (torch.complex128 if f64 else torch.complex64)
        if avg and n == 0:
            raise ValueError(f"output={mode!r} averages over the trials and there are n=0 of them")
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=x.device)
        elif tuple(out.shape) != shape or out.dtype != dtype or out.device != x.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {dtype} tensor of shape {shape} on {x.device}")
        if out.numel() == 0:
            return out
        work = _lib.workspace(L.isd_tfr_work_bytes(self._h, n, Cn, T, m, int(f64)), x.device)
        with torch.cuda.device(x.device):
            fn = _lib.typed("isd_tfr_cwt", x.dtype)
            _lib.check(fn(self._h, x.data_ptr(), out.data_ptr(), n, Cn, T, m, work.data_ptr(), _lib.stream()))
        return out


@functools.lru_cache(maxsize=16)
def _cached_plan(n_taps, taps_bytes, decim, device_index):
    with torch.cuda.device(device_index):
        return TfrPlan(n_taps, np.frombuffer(taps_bytes, dtype=np.complex128), decim)


def _check_input(x, ndim, name):
    """-> (x as a tensor or ndarray, is_tensor); TypeError for CPU tensors and non-float dtypes, ValueError for the wrong rank."""
    x, is_tensor = _lib.check_array(x, name)
    if x.ndim != ndim:
        raise ValueError(f"{name} must have {ndim} axes, got shape {tuple(x.shape)}")
    return x, is_tensor


def cwt(X, Ws, use_fft=True, mode="same", decim=1):
    """Convolve the rows of ``X`` [rows, T] with the complex tap vectors ``Ws`` (odd lengths, none longer than T)
    -> complex [rows, F, ceil(T / decim)]:  out[r, j] = np.convolve(X[r], Ws[j], 'same')[::decim].  ``use_fft`` is
    accepted and ignored (the product is dense); a ``mode`` other than 'same' raises NotImplementedError."""
    if mode != "same":
        raise NotImplementedError(f"mode={mode!r}: only 'same' is provided")
    decim = _check_decim(decim)
    X, is_tensor = _check_input(X, 2, "X")
    Ws = [np.ascontiguousarray(W, dtype=np.complex128) for W in Ws]
    if any(W.ndim != 1 for W in Ws):
        raise ValueError("every wavelet must be a 1-D array of taps")
    n_taps = tuple(int(W.shape[0]) for W in Ws)
    _check_taps(n_taps, int(X.shape[-1]))
    xd = _lib.to_device(X, is_tensor, "tfr.cwt")
    plan = _cached_plan(n_taps, np.concatenate(Ws).tobytes(), decim, xd.device.index)
    out = plan(xd[None], "complex")[0]
    return out if is_tensor else out.cpu().numpy()


def tfr_array_morlet(data, sfreq, freqs, n_cycles=7.0, zero_mean=True, use_fft=True, decim=1, output="complex",
                     n_jobs=None, *, verbose=None):
    """Morlet time-frequency transform of ``data`` [n, C, T] -- argument order and defaults of
    ``mne.time_frequency.tfr_array_morlet``.  With F = len(freqs) and T_out = ceil(T / decim):

    'complex' -> complex [n, C, F, T_out]; 'power' -> |z|^2 and 'phase' -> angle(z), real [n, C, F, T_out];
    'avg_power' -> the mean over trials of |z|^2 and 'itc' -> |mean over trials of z / |z||, real [C, F, T_out];
    'avg_power_itc' -> complex [C, F, T_out], avg_power + 1j itc.  The averaged outputs write nothing per trial and
    sum in fp64; in 'itc' a sample with |z| = 0 contributes 0 (MNE yields NaN there).  'phase' is atan2(im, re) in
    the kernel's epilogue, from an fp64 product for both input types.

    ndarray in -> computed in fp64 on the GPU -> float64 / complex128 ndarray out; float32 / float64 CUDA tensor in ->
    CUDA tensor of the matching real or complex dtype out.  ``use_fft``, ``n_jobs`` and ``verbose`` are accepted and
    ignored.  n = 0 gives an empty per-trial result and is an error for the averaged ones."""
    if output not in OUTPUTS:
        raise ValueError(f"output={output!r} (need one of {', '.join(OUTPUTS)})")
    decim = _check_decim(decim)
    data, is_tensor = _check_input(data, 3, "data")
    sfreq, freqs, n_cycles = _freqs_cycles(sfreq, freqs, n_cycles)
    if freqs.size > MAX_FREQS:
        raise NotImplementedError(f"{freqs.size} frequencies: at most MAX_FREQS = {MAX_FREQS} are provided")
    n, T = int(data.shape[0]), int(data.shape[2])
    n_taps, taps_bytes = _cached_morlet(sfreq, freqs.tobytes(), n_cycles.tobytes(), bool(zero_mean))
    _check_taps(n_taps, T)
    if n == 0 and output in ("avg_power", "itc", "avg_power_itc"):
        raise ValueError(f"output={output!r} averages over the trials and there are n=0 of them")
    xd = _lib.to_device(data, is_tensor, "tfr_array_morlet")
    plan = _cached_plan(n_taps, taps_bytes, decim, xd.device.index)
    out = plan(xd, output)
    return out if is_tensor else out.cpu().numpy()
