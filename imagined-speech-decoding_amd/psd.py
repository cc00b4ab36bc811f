"""Welch power spectral density on the GPU: the PSD step of the reference's artifact analysis.

``psd_array_welch(x, sfreq, ...)`` has the argument order and defaults of ``mne.time_frequency.psd_array_welch``,
which is what ``raw.compute_psd(method='welch')`` runs (scripts/artifact_analysis.py:45), and returns
``(psds, freqs)``: a density in (unit of x)² / Hz over the bins with ``fmin <= f <= fmax``.  With ``isd_amd.ICA`` it
answers the question that script asks of a component -- how much of its power is muscle or line noise -- without
leaving the card: ``band_power(*psd_array_welch(ica.get_sources(X), 250), relative=True)``.

MNE is not vendored in the reference and is not installed here.  The behaviour is restated from its documentation and
pinned by scipy (``scipy.signal.welch`` / ``scipy.signal.spectrogram`` with ``scaling='density'``, no boundary
extension, no padding); parity with MNE itself is not pinned.  The segment bookkeeping, the window and every argument
check are host work (``welch_design``, pure NumPy); the transform runs in libisd_hip.so (csrc/psd.hip) as a dense
product over the kept bins.  There is no CPU fallback.  Not provided: multitaper estimation, complex output,
``n_fft > 2048``, a gradient.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .constants import BANDS_5, band_edges

MAX_N_FFT = 2048                     # isd_psd_plan_create: 2 <= n_fft <= 2048

WelchDesign = namedtuple("WelchDesign", "n_fft n_per_seg n_overlap step n_segments k_lo k_hi freqs window scale")


def periodic_window(name, n):
    """'hamming' / 'hann' as ``scipy.signal.get_window(name, n)`` returns them (periodic, float64)."""
    if name not in ("hamming", "hann"):
        raise NotImplementedError(f"window={name!r}: only 'hamming', 'hann' or an array of taps is provided")
    if n <= 1:
        return np.ones(n)
    a = 0.54 if name == "hamming" else 0.5
    return a - (1.0 - a) * np.cos(2.0 * np.pi * np.arange(n) / n)


def welch_design(sfreq, n_times, fmin=0, fmax=np.inf, n_fft=256, n_overlap=0, n_per_seg=None, window="hamming"):
    """Resolve the arguments of ``psd_array_welch`` for rows of ``n_times`` samples; never touches the GPU.

    -> WelchDesign(n_fft, n_per_seg, n_overlap, step, n_segments, k_lo, k_hi, freqs, window, scale): the kept bins are
    k_lo .. k_hi of the one-sided transform, ``freqs`` [K] their frequencies, ``window`` [n_per_seg] the taps and
    ``scale`` [K] the factor c_k / (sfreq Σw²) that turns |X_k|² into a density (c_k = 2, but 1 at k = 0 and at the
    Nyquist bin of an even n_fft).  ``n_per_seg=None`` means n_fft; n_per_seg is clamped to n_fft and to n_times."""
    sfreq, n_times, n_fft, n_overlap = float(sfreq), int(n_times), int(n_fft), int(n_overlap)
    if not sfreq > 0:
        raise ValueError(f"sfreq={sfreq!r} (need > 0)")
    if n_fft < 2:
        raise ValueError(f"n_fft={n_fft} (need >= 2)")
    if n_per_seg is None and n_fft > n_times:
        raise ValueError(f"n_fft={n_fft} is longer than the {n_times} samples and n_per_seg is None: give n_per_seg "
                         "to zero-pad shorter segments")
    n_per_seg = n_fft if n_per_seg is None or int(n_per_seg) > n_fft else int(n_per_seg)
    n_per_seg = min(n_per_seg, n_times)
    if n_per_seg < 1:
        raise ValueError(f"n_per_seg={n_per_seg} (need >= 1; the rows have {n_times} samples)")
    if not 0 <= n_overlap < n_per_seg:
        raise ValueError(f"n_overlap={n_overlap} (need 0 <= n_overlap < n_per_seg={n_per_seg})")
    if isinstance(window, str):
        taps = periodic_window(window, n_per_seg)
    else:
        taps = np.ascontiguousarray(window, dtype=np.float64)
        if taps.ndim != 1 or taps.shape[0] != n_per_seg:
            raise ValueError(f"window must have n_per_seg={n_per_seg} taps, got shape {taps.shape}")
        if not np.all(np.isfinite(taps)) or not np.sum(taps * taps) > 0:
            raise ValueError("window taps must be finite and not all zero")
    step = n_per_seg - n_overlap
    freqs = np.fft.rfftfreq(n_fft, 1.0 / sfreq)                    # k sfreq / n_fft, as scipy forms it
    keep = np.flatnonzero((freqs >= fmin) & (freqs <= fmax))
    if keep.size == 0:
        raise ValueError(f"no frequency bin in [{fmin}, {fmax}] Hz (bin width {sfreq / n_fft:g} Hz)")
    k_lo, k_hi = int(keep[0]), int(keep[-1])
    k = np.arange(k_lo, k_hi + 1)
    ck = np.where((k == 0) | (2 * k == n_fft), 1.0, 2.0)
    scale = ck / (sfreq * np.sum(taps * taps))
    return WelchDesign(n_fft, n_per_seg, n_overlap, step, (n_times - n_per_seg) // step + 1, k_lo, k_hi,
                       freqs[k_lo:k_hi + 1], taps, scale)


def median_bias(n):
    """Bias of the median of n chi-square (2 degrees of freedom) variates against their mean:
    1 + Σ_{i=1..(n−1)//2} (1/(2i+1) − 1/(2i)), what ``scipy.signal.welch(average='median')`` divides by."""
    ii_2 = 2.0 * np.arange(1.0, (int(n) - 1) // 2 + 1)
    return float(1.0 + np.sum(1.0 / (ii_2 + 1.0) - 1.0 / ii_2))


class WelchPlan(_lib.Handle):
    """The device tables of one (n_fft, n_per_seg, n_overlap, bins, window, sfreq, remove_dc) on one device."""
    _destroy = "isd_psd_plan_destroy"

    def __init__(self, n_fft, n_per_seg, n_overlap, k_lo, k_hi, window, sfreq, remove_dc):
        self._create("isd_psd_plan_create", n_fft, n_per_seg, n_overlap, k_lo, k_hi, _lib.double_array(window),
                     float(sfreq), int(bool(remove_dc)))
        self.bins = _lib.lib().isd_psd_plan_bins(self._h)

    def __call__(self, x, per_segment=False):
        """x contiguous CUDA [rows, T] (f32 / f64) -> [rows, K], or per_segment [rows, K, S], of x's dtype."""
        L = _lib.lib()
        rows, T = x.shape
        S = int(L.isd_psd_plan_segments(self._h, T))
        f64 = x.dtype == torch.float64
        out = torch.empty((rows, self.bins, S) if per_segment else (rows, self.bins), dtype=x.dtype, device=x.device)
        if rows == 0:
            return out
        work = _lib.workspace(L.isd_psd_work_bytes(self._h, rows, T, int(f64)), x.device)
        with torch.cuda.device(x.device):
            fn = _lib.typed("isd_psd_welch", x.dtype)
            _lib.check(fn(self._h, x.data_ptr(), out.data_ptr(), rows, T, int(bool(per_segment)), work.data_ptr(),
                          _lib.stream()))
        return out


@functools.lru_cache(maxsize=16)
def _cached_plan(n_fft, n_per_seg, n_overlap, k_lo, k_hi, window_bytes, sfreq, remove_dc, device_index):
    with torch.cuda.device(device_index):
        return WelchPlan(n_fft, n_per_seg, n_overlap, k_lo, k_hi, np.frombuffer(window_bytes, dtype=np.float64),
                         sfreq, remove_dc)


@functools.lru_cache(maxsize=64)
def _cached_design(sfreq, n_times, fmin, fmax, n_fft, n_overlap, n_per_seg, window, taps_bytes):
    """welch_design by value: ``window`` a name, or the taps' shape with their bytes in ``taps_bytes``."""
    if taps_bytes is not None:
        window = np.frombuffer(taps_bytes, dtype=np.float64).reshape(window)
    return welch_design(sfreq, n_times, fmin, fmax, n_fft, n_overlap, n_per_seg, window)


def psd_array_welch(x, sfreq, fmin=0, fmax=np.inf, n_fft=256, n_overlap=0, n_per_seg=None, n_jobs=None,
                    average="mean", window="hamming", remove_dc=True, *, output="power", verbose=None):
    """Welch PSD of the last axis of ``x`` [..., T] -- argument order and defaults of
    ``mne.time_frequency.psd_array_welch``.  -> (psds, freqs): psds [..., K] for ``average='mean'`` / ``'median'``,
    [..., K, S] for ``average=None``; freqs a float64 ndarray [K].  ndarray in -> computed in fp64 on the GPU ->
    float64 ndarray out; float32 / float64 CUDA tensor in -> CUDA tensor of that dtype out.  ``n_jobs`` and
    ``verbose`` are accepted and ignored; ``output='complex'`` raises NotImplementedError."""
    if output != "power":
        raise NotImplementedError(f"output={output!r}: only 'power' is provided")
    if average not in ("mean", "median", None):
        raise ValueError(f"average={average!r} (need 'mean', 'median' or None)")
    x, is_tensor = _lib.check_array(x, "x")
    if x.ndim < 1:
        raise ValueError("x must have a time axis")
    lead, T = tuple(x.shape[:-1]), int(x.shape[-1])
    if isinstance(window, str):
        d = _cached_design(float(sfreq), T, float(fmin), float(fmax), int(n_fft), int(n_overlap), n_per_seg, window,
                           None)
    else:
        taps = np.ascontiguousarray(window, dtype=np.float64)
        d = _cached_design(float(sfreq), T, float(fmin), float(fmax), int(n_fft), int(n_overlap), n_per_seg,
                           taps.shape, taps.tobytes())
    if d.n_fft > MAX_N_FFT:
        raise NotImplementedError(f"n_fft={d.n_fft}: at most {MAX_N_FFT} is provided")
    xd = _lib.to_device(x, is_tensor, "psd_array_welch")
    plan = _cached_plan(d.n_fft, d.n_per_seg, d.n_overlap, d.k_lo, d.k_hi, d.window.tobytes(), float(sfreq),
                        bool(remove_dc), xd.device.index)
    K, S = d.k_hi - d.k_lo + 1, d.n_segments
    out = plan(xd.reshape(-1, T), per_segment=average != "mean")
    if average == "mean":
        out = out.reshape(lead + (K,))
    elif average is None:
        out = out.reshape(lead + (K, S))
    else:                                                          # np.median: the two middle values averaged
        v = torch.sort(out, dim=-1).values
        out = ((v[..., (S - 1) // 2] + v[..., S // 2]) / (2.0 * median_bias(S))).reshape(lead + (K,))
    return (out if is_tensor else out.cpu().numpy()), d.freqs.copy()          # the design is shared between calls


def psd_array_multitaper(*args, **kwargs):
    raise NotImplementedError("multitaper estimation is not provided: use psd_array_welch")


def band_power(psds, freqs, bands=BANDS_5, relative=False):
    """psds [..., K] (tensor or ndarray) at ``freqs`` [K] -> [..., n_bands]: per band (name, lo, hi) the sum of the
    density over lo <= f <= hi times the bin width; ``relative`` divides by the total over ``freqs``."""
    freqs = np.asarray(freqs, dtype=np.float64)
    if freqs.ndim != 1 or psds.shape[-1] != freqs.shape[0]:
        raise ValueError(f"psds [..., K] and freqs [K] disagree: {tuple(psds.shape)} against {freqs.shape}")
    df = float(freqs[1] - freqs[0]) if freqs.size > 1 else 1.0
    cols = []
    for lo, hi in band_edges(bands):
        idx = np.flatnonzero((freqs >= lo) & (freqs <= hi))
        cols.append(psds[..., int(idx[0]):int(idx[-1]) + 1].sum(-1) * df if idx.size else psds[..., :1].sum(-1) * 0.0)
    out = torch.stack(cols, dim=-1) if isinstance(psds, torch.Tensor) else np.stack(cols, axis=-1)
    if relative:
        out = out / (psds.sum(-1) * df)[..., None]
    return out
