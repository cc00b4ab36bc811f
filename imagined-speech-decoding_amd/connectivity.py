"""Cross-spectral density and spectral connectivity on the GPU: the frequency-resolved cross-channel estimates next to
``psd_array_welch`` (one channel, per frequency) and the trial covariances of ``CSP`` / ``riemann`` (all channels,
broadband).

``csd_array_welch(x, sfreq, ...)`` -> ``(csd, freqs)``: x [n, C, T] (or [C, T]) -> the Welch cross-spectral density
``S[i, j] = mean X_i conj(X_j)`` over the bins with ``fmin <= f <= fmax``, complex, [n, K, C, C] for
``average='segments'`` (the mean over a trial's segments) or [K, C, C] for ``average='trials'`` (over every segment of
every trial).  In scipy's terms ``S[i, j]`` is ``scipy.signal.csd(x_j, x_i, window=..., nperseg=..., noverlap=...,
nfft=..., detrend='constant', scaling='density')`` -- scipy conjugates its first argument -- and the diagonal is
``psd_array_welch`` with the same window.

``spectral_connectivity(x, sfreq, method=...)`` -> ``(con, freqs)`` derives from it

    'cohy'  = S_ij / sqrt(S_ii S_jj)        'coh' = |cohy|        'imcoh' = Im cohy

and from a second pass in which every segment spectrum is first divided by its modulus, E = mean u_i conj(u_j) over
the N (trial, segment) pairs averaged,

    'plv' = |E|        'ciplv' = |Im E| / sqrt(1 - (Re E)^2)        'ppc' = (N |E|^2 - 1) / (N - 1).

The names and formulas follow the documentation of mne-connectivity (``spectral_connectivity_epochs``); that library is
not installed here and **parity with it is unpinned**: the tests pin the formulas above against a NumPy restatement and
scipy (``scipy.signal.csd`` / ``coherence``).  Multitaper and wavelet modes and ``indices=`` are not provided here
and raise NotImplementedError by name, and so do the phase-lag measures ('pli', 'dpli', 'wpli', 'wpli2_debiased'):
they are sums over samples of sign(Im s), |Im s| and (Im s)^2 per channel pair, not Hermitian products of segment
spectra, so the Welch route cannot form them.  They live in ``spectral_connectivity_time`` below.

``spectral_connectivity_time(data, freqs, method=..., sfreq=...)`` -> ``(con, freqs)`` is the time-resolved estimate,
one [F, C, C] map PER TRIAL from the Morlet cross-spectrum averaged over the trial's samples (hundreds of them, where a
trial has three to five Welch segments): 'coh', 'imcoh', 'plv', 'ciplv' and the phase-lag family 'pli', 'dpli', 'wpli',
'wpli2_debiased'.  The complex map comes from ``tfr``'s plan in trial chunks of at most CONTIME_CHUNK_BYTES and one
fused kernel (csrc/contime.hip) turns each chunk into the measures: one pass over the map per pair of channel tiles,
a compensated cross product for Im s (the sign of a nearly in-phase pair is what pli and dpli are made of), fp64
sums.  In torch ops it is a [chunk, F, C, C, T] complex intermediate and five or six passes over it.  The names follow
``mne_connectivity.spectral_connectivity_time``; **parity with it is unpinned** as well.

The segment bookkeeping, the window and the argument checks are ``psd.welch_design``; the data-sized work runs in
libisd_hip.so (csrc/csd.hip: segment spectra as a dense product on the plan's tables, then a Hermitian product per
bin); the step from the density to a measure is elementwise torch ops on the device.  A call that asks for 'ciplv'
runs its unit-modulus pass in fp64 for float32 input too.  There is no CPU fallback.
ndarray in -> computed in fp64 on the GPU -> float64 / complex128 ndarray out; float32 / float64 CUDA tensor in ->
CUDA tensor of the matching real or complex dtype out.

``envelope_correlation(data, orthogonalize='pairwise', log=False, absolute=True)`` -> [n, C, C] is the amplitude side:
the orthogonalised power-envelope correlation of Hipp et al. 2012, which does not mistake volume conduction for
coupling.  Per trial, with z [C, T] the analytic signal (``analytic.hilbert`` of real data), m = |z|, u = conj(z) / m
(0 where m = 0), e = log(m^2) if ``log`` else m, ec = e - mean_t e, se = |ec|_2 (1 where it is 0):

    o[l, j, t] = |Im(z[l, t] u[j, t])|  (log(o^2) if ``log``),  oc = o - mean_t o,  so = |oc|_2 (1 where it is 0)
    corr[l, j] = sum_t oc[l, j, t] ec[j, t] / (se[j] so[l, j]),  corr[l, l] = 0
    result     = (A + A^T) / 2,  A = |corr| if ``absolute`` else corr

and with ``orthogonalize=False`` corr[l, j] = sum_t ec[l, t] ec[j, t] / (se[l] se[j]), np.corrcoef of the envelopes
(no abs, no symmetrisation).  The name and the arguments follow ``mne_connectivity.envelope_correlation``; that library
is not installed here and **parity with it is unpinned**: the tests pin the formulas above against a NumPy restatement.
It is one fused kernel (csrc/envcorr.hip) that reads z once per pair of channel tiles and writes [n, C, C]; in torch
ops it is an [n, C, C, T] intermediate and several passes over it.
"""

import numpy as np
import torch

from . import _lib
from . import tfr as _tfr
from .analytic import hilbert_device
from .constants import BANDS_5, band_edges
from .psd import MAX_N_FFT, _cached_design, _cached_plan

MAX_CHANNELS = 128                   # isd_csd_welch_*: 1 <= C <= 128
CSD_CHUNK_BYTES = None               # bound on the spectra workspace of one trial chunk inside the library call
#                                      (None: the library's 256 MiB)
CON_CHUNK_BYTES = 256 << 20          # spectral_connectivity(average='segments'): bound on one [chunk, K, C, C] density

DENSITY_METHODS = ("coh", "cohy", "imcoh")
PHASE_METHODS = ("plv", "ciplv", "ppc")
METHODS = DENSITY_METHODS + PHASE_METHODS
NOT_PROVIDED = ("pli", "dpli", "wpli", "wpli2_debiased", "pli2_unbiased", "gc", "gc_tr", "mic", "mim", "cacoh")


def _check_input(x):
    """-> (x as [n, C, T], is_tensor, squeeze): every check that needs no GPU."""
    x, is_tensor = _lib.check_array(x, "x")
    if x.ndim not in (2, 3):
        raise ValueError(f"x must be [n, C, T] or [C, T], got {tuple(x.shape)}")
    squeeze = x.ndim == 2
    if squeeze:
        x = x[None]
    if not 1 <= x.shape[1] <= MAX_CHANNELS:
        raise NotImplementedError(f"{x.shape[1]} channels: 1 to {MAX_CHANNELS} are provided")
    return x, is_tensor, squeeze


def _design(T, sfreq, fmin, fmax, n_fft, n_overlap, n_per_seg, window):
    if isinstance(window, str):
        d = _cached_design(float(sfreq), T, float(fmin), float(fmax), int(n_fft), int(n_overlap), n_per_seg, window,
                           None)
    else:
        taps = np.ascontiguousarray(window, dtype=np.float64)
        d = _cached_design(float(sfreq), T, float(fmin), float(fmax), int(n_fft), int(n_overlap), n_per_seg,
                           taps.shape, taps.tobytes())
    if d.n_fft > MAX_N_FFT:
        raise NotImplementedError(f"n_fft={d.n_fft}: at most {MAX_N_FFT} is provided")
    return d


def csd_launch(plan, x, over_trials, unit_modulus=False, out=None):
    """One library call: x contiguous CUDA [n, C, T] (f32 / f64) -> complex [n, K, C, C], or over_trials [K, C, C];
    ``out`` (a contiguous complex tensor of that shape) receives the result if given."""
    L = _lib.lib()
    n, Cc, T = x.shape
    f64 = x.dtype == torch.float64
    K = plan.bins
    shape = (K, Cc, Cc) if over_trials else (n, K, Cc, Cc)
    cdtype = torch.complex128 if f64 else torch.complex64
    if out is None:
        out = torch.empty(shape, dtype=cdtype, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != cdtype or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"out must be a contiguous {cdtype} tensor of shape {shape} on {x.device}")
    if n == 0:
        return out.zero_() if over_trials else out
    L.isd_csd_chunk_bytes(0 if CSD_CHUNK_BYTES is None else int(CSD_CHUNK_BYTES))
    work = _lib.workspace(L.isd_csd_work_bytes(plan._h, n, Cc, T, int(bool(over_trials)), int(f64)), x.device)
    with torch.cuda.device(x.device):
        fn = _lib.typed("isd_csd_welch", x.dtype)
        _lib.check(fn(plan._h, x.data_ptr(), out.data_ptr(), n, Cc, T, int(bool(over_trials)),
                      int(bool(unit_modulus)), work.data_ptr(), _lib.stream()))
    return out


def _plan_for(d, sfreq, remove_dc, device):
    return _cached_plan(d.n_fft, d.n_per_seg, d.n_overlap, d.k_lo, d.k_hi, d.window.tobytes(), float(sfreq),
                        bool(remove_dc), device.index)


def csd_array_welch(x, sfreq, fmin=0, fmax=np.inf, n_fft=256, n_overlap=0, n_per_seg=None, window="hann",
                    remove_dc=True, average="segments"):
    """Welch cross-spectral density of x [n, C, T] ([C, T] is n = 1) -> (csd, freqs): csd complex [n, K, C, C] for
    ``average='segments'``, [K, C, C] for ``average='trials'``; freqs a float64 ndarray [K].  A density,
    ``S[i, j] = mean X_i conj(X_j) c_k / (sfreq Σw²)``; the Welch arguments are those of ``psd_array_welch``.
    ``csd[..., i, j] == conj(csd[..., j, i])`` bit for bit and the diagonal is real."""
    if average not in ("segments", "trials"):
        raise ValueError(f"average={average!r} (need 'segments' or 'trials')")
    x, is_tensor, squeeze = _check_input(x)
    d = _design(int(x.shape[-1]), sfreq, fmin, fmax, n_fft, n_overlap, n_per_seg, window)
    xd = _lib.to_device(x, is_tensor, "connectivity")
    out = csd_launch(_plan_for(d, sfreq, remove_dc, xd.device), xd, average == "trials")
    if squeeze and average == "segments":
        out = out[0]
    return (out if is_tensor else out.cpu().numpy()), d.freqs.copy()


def band_bins(freqs, bands=BANDS_5):
    """Per band (name, lo, hi) the indices of ``freqs`` with lo <= f <= hi (both ends inclusive, as ``band_power``)."""
    freqs = np.asarray(freqs, dtype=np.float64)
    return [np.flatnonzero((freqs >= lo) & (freqs <= hi)) for lo, hi in band_edges(bands)]


def check_methods(method):
    """-> (list of names, whether a single name was given); raises by name for what is not provided."""
    single = isinstance(method, str)
    names = [method] if single else list(method)
    if not names:
        raise ValueError("method is empty")
    for m in names:
        if m in NOT_PROVIDED:
            raise NotImplementedError(f"method={m!r} is not a Hermitian product of segment spectra and is not "
                                      f"provided; provided: {', '.join(METHODS)}")
        if m not in METHODS:
            raise ValueError(f"method={m!r} (provided: {', '.join(METHODS)})")
    return names, single


def _measure(name, S, E, N):
    """One measure from the density S and / or the mean phase product E ([..., K, C, C] complex tensors)."""
    if name in DENSITY_METHODS:
        dg = torch.diagonal(S, dim1=-2, dim2=-1).real
        cohy = S / torch.sqrt(dg[..., :, None] * dg[..., None, :])
        return cohy if name == "cohy" else (cohy.abs() if name == "coh" else cohy.imag)
    if name == "plv":
        return E.abs()
    if name == "ciplv":                                            # 1 - Re^2 as (1 - Re)(1 + Re): 1 - Re is exact near 1
        return E.imag.abs() / torch.sqrt((1.0 - E.real) * (1.0 + E.real))
    return (N * (E.real * E.real + E.imag * E.imag) - 1.0) / (N - 1.0)          # ppc


def _band_mean(v, bins):
    """[..., K, C, C] -> [..., n_bands, C, C]: the mean over each band's bins."""
    return torch.stack([v[..., torch.as_tensor(b, device=v.device), :, :].mean(-3) for b in bins], dim=-3)


def spectral_connectivity(x, sfreq, method="coh", fmin=0, fmax=np.inf, n_fft=256, n_overlap=0, n_per_seg=None,
                          window="hann", remove_dc=True, average="trials", faverage=False, bands=None, mode="welch",
                          indices=None):
    """Connectivity of x [n, C, T] between every pair of channels -> (con, freqs).

    ``method``: one of 'coh', 'cohy', 'imcoh', 'plv', 'ciplv', 'ppc' or a list of them (a list returns a list; all
    share one density pass and / or one unit-modulus pass).  ``average='trials'`` estimates over every segment of every
    trial, con [K, C, C]; ``'segments'`` per trial over its own segments, con [n, K, C, C] (computed in trial chunks
    of at most CON_CHUNK_BYTES).  ``faverage=True`` averages the measure over the kept bins of each band of ``bands``
    (default BANDS_5): con [..., n_bands, C, C] and freqs the bands' mean frequencies; a band without a kept bin is an
    error.  'cohy' is complex, the others real.  'ppc' needs at least two (trial, segment) pairs.  The diagonal of
    'ciplv' is 0 / 0 = NaN; when 'ciplv' is asked for, the unit-modulus pass runs in fp64 for float32 input too
    (its denominator 1 - (Re E)^2 amplifies the rounding of E) and 'plv' / 'ppc' of the same call come from it.  Names and formulas follow mne-connectivity's documentation; parity with that library is
    unpinned (it is not installed here)."""
    names, single = check_methods(method)
    if mode != "welch":
        raise NotImplementedError(f"mode={mode!r}: only the Welch estimate is provided (no multitaper, no wavelets)")
    if indices is not None:
        raise NotImplementedError("indices= is not provided: every pair of channels is computed")
    if average not in ("segments", "trials"):
        raise ValueError(f"average={average!r} (need 'segments' or 'trials')")
    x, is_tensor, _ = _check_input(x)
    n, Cc, T = (int(v) for v in x.shape)
    d = _design(T, sfreq, fmin, fmax, n_fft, n_overlap, n_per_seg, window)
    K = d.k_hi - d.k_lo + 1
    freqs = d.freqs.copy()
    bins = None
    if faverage:
        bands = BANDS_5 if bands is None else bands
        bins = band_bins(freqs, bands)
        for b, band in zip(bins, bands):
            if b.size == 0:
                raise ValueError(f"band {band!r} holds no kept frequency bin")
        freqs = np.array([d.freqs[b].mean() for b in bins])
    over = average == "trials"
    N = float(n * d.n_segments if over else d.n_segments)
    if "ppc" in names and N < 2:
        raise ValueError("method='ppc' needs at least two (trial, segment) pairs")
    need_s = any(m in DENSITY_METHODS for m in names)
    need_e = any(m in PHASE_METHODS for m in names)

    def run(xd):
        plan = _plan_for(d, sfreq, remove_dc, xd.device)
        S = csd_launch(plan, xd, over) if need_s else None
        # ciplv divides by d = 1 - (Re E)^2 and so multiplies the error of E by up to 1 / d: nearly locked pairs
        # (d ~ 1e-5) would keep two digits of a float32 E.  When it is asked for, the one unit-modulus pass runs in
        # fp64 whatever the input type, and the phase measures are rounded to the input's type at the end.
        xe = xd.double() if "ciplv" in names else xd
        E = csd_launch(plan, xe, over, unit_modulus=True) if need_e else None
        vals = [_measure(m, S, E, N) for m in names]
        vals = [v if m in DENSITY_METHODS else v.to(xd.dtype) for m, v in zip(names, vals)]
        return [_band_mean(v, bins) for v in vals] if faverage else vals

    if over or n == 0:
        res = run(_lib.to_device(x, is_tensor, "connectivity"))
    else:
        per = K * Cc * Cc * 16 * (int(need_s) + int(need_e))
        step = max(1, CON_CHUNK_BYTES // per)
        parts = [run(_lib.to_device(x[s:s + step], is_tensor, "connectivity")) for s in range(0, n, step)]
        res = [torch.cat([p[i] for p in parts]) for i in range(len(names))]
    if not is_tensor:
        res = [r.cpu().numpy() for r in res]
    return (res[0] if single else res), freqs


# ---------------------------------------------------------------------------------------------- envelope correlation
ENVCORR_CHUNK = 16                   # samples per staged chunk of the pair kernel (kEnvChunk of csrc/envcorr.hip)
ENV_LOG, ENV_ABSOLUTE, ENV_PLAIN = 1, 2, 4
_REAL_OF = {torch.complex64: torch.float32, torch.complex128: torch.float64}
_ENV_DTYPES = (torch.float32, torch.float64, torch.complex64, torch.complex128)


def envcorr_launch(z, flags, out=None):
    """One library call: z contiguous complex CUDA [n, C, T] -> real [n, C, C]; ``out`` (a contiguous real tensor of
    that shape) receives the result if given."""
    L = _lib.lib()
    n, Cc, T = z.shape
    rdtype = _REAL_OF[z.dtype]
    f64 = rdtype == torch.float64
    if out is None:
        out = torch.empty((n, Cc, Cc), dtype=rdtype, device=z.device)
    elif tuple(out.shape) != (n, Cc, Cc) or out.dtype != rdtype or not out.is_contiguous() or out.device != z.device:
        raise ValueError(f"out must be a contiguous {rdtype} tensor of shape {(n, Cc, Cc)} on {z.device}")
    if n == 0:
        return out
    work = _lib.workspace(L.isd_envcorr_work_bytes(n, Cc, T, int(f64)), z.device)
    with torch.cuda.device(z.device):
        fn = _lib.typed("isd_envcorr", rdtype)
        _lib.check(fn(torch.view_as_real(z).data_ptr(), out.data_ptr(), n, Cc, T, int(flags), work.data_ptr(),
                      _lib.stream()))
    return out


def envelope_correlation(data, orthogonalize="pairwise", log=False, absolute=True):
    """Pairwise envelope correlation of data [n, C, T] -> [n, C, C] real ([C, T] -> [C, C]); the formulas are in the
    module's docstring.

    ``data`` real goes through ``analytic.hilbert`` first (as mne-connectivity does); complex data (a complex64 /
    complex128 CUDA tensor or a complex ndarray) is taken as the analytic signal as it is.  ``orthogonalize`` is
    'pairwise' or False.  1 <= C <= MAX_CHANNELS, T >= 1.  The orthogonalised result is symmetric bit for bit with an
    exactly zero diagonal; a dead (all-zero) channel gives a row and a column of zeros for ``log=False``; with
    ``log=True`` an exact zero of |z| or of an orthogonalised envelope makes the entries it enters NaN and no other.
    ndarray in -> the fp64 route -> float64 ndarray out.  Names follow ``mne_connectivity.envelope_correlation``;
    parity with that library is unpinned (it is not installed here)."""
    if not (orthogonalize is False or (isinstance(orthogonalize, str) and orthogonalize == "pairwise")):
        raise ValueError(f"orthogonalize={orthogonalize!r} (need 'pairwise' or False)")
    is_tensor = isinstance(data, torch.Tensor)
    if is_tensor:
        data, _ = _lib.check_array(data, "data", _ENV_DTYPES)
        is_complex = data.is_complex()
    else:
        data = np.asarray(data)
        if data.dtype.kind not in "fc":
            raise TypeError("data must be floating point or complex")
        is_complex = data.dtype.kind == "c"
    if data.ndim not in (2, 3):
        raise ValueError(f"data must be [n, C, T] or [C, T], got {tuple(data.shape)}")
    squeeze = data.ndim == 2
    if squeeze:
        data = data[None]
    n, Cc, T = (int(v) for v in data.shape)
    if not 1 <= Cc <= MAX_CHANNELS:
        raise NotImplementedError(f"{Cc} channels: 1 to {MAX_CHANNELS} are provided")
    if T < 1:
        raise ValueError("data must have at least one sample")
    if is_tensor:
        z = data.resolve_conj().contiguous()
    else:
        z = _lib.to_device(data, False, "connectivity", dtype=np.complex128 if is_complex else np.float64)
    if not is_complex:
        z = hilbert_device(z, T)
    flags = (ENV_LOG if log else 0) | (ENV_ABSOLUTE if absolute else 0) | (0 if orthogonalize else ENV_PLAIN)
    out = envcorr_launch(z, flags)
    if squeeze:
        out = out[0]
    return out if is_tensor else out.cpu().numpy()


# --------------------------------------------------------------------------------- time-resolved spectral connectivity
CONTIME_CHUNK_BYTES = 256 << 20      # spectral_connectivity_time: bound on the complex map [chunk, C, F, T_out] alive
CONTIME_METHODS = ("coh", "imcoh", "plv", "ciplv", "pli", "dpli", "wpli", "wpli2_debiased")   # bit m of methods_mask
CONTIME_MULTIVARIATE = ("cacoh", "mic", "mim", "gc", "gc_tr")


def contime_mask(names):
    """The methods_mask of a list of CONTIME_METHODS names; the library stores the measures in bit order."""
    mask = 0
    for m in names:
        mask |= 1 << CONTIME_METHODS.index(m)
    return mask


def contime_launch(z, methods_mask, t0, t1, out=None, average=False):
    """One library call: z contiguous complex CUDA [n, C, F, T_out] -> real [M, n, F, C, C] ([M, F, C, C] with
    ``average``): the M measures of ``methods_mask`` (bit m = CONTIME_METHODS[m]) in bit order over the samples
    t0 <= t < t1; ``out`` (a contiguous real tensor of that shape) receives the result if given."""
    if not (isinstance(z, torch.Tensor) and z.is_cuda and z.dtype in _REAL_OF and z.ndim == 4 and z.is_contiguous()):
        raise ValueError("z must be a contiguous complex64 / complex128 CUDA tensor [n, C, F, T_out]")
    n, Cc, F, T = z.shape
    rdtype = _REAL_OF[z.dtype]
    M = bin(int(methods_mask) & 0xFF).count("1")
    shape = (M, F, Cc, Cc) if average else (M, n, F, Cc, Cc)
    if out is None:
        out = torch.empty(shape, dtype=rdtype, device=z.device)
    elif tuple(out.shape) != shape or out.dtype != rdtype or not out.is_contiguous() or out.device != z.device:
        raise ValueError(f"out must be a contiguous {rdtype} tensor of shape {shape} on {z.device}")
    if n == 0 and not average:
        return out
    with torch.cuda.device(z.device):
        fn = _lib.typed("isd_contime", rdtype)
        _lib.check(fn(torch.view_as_real(z).data_ptr(), out.data_ptr(), n, Cc, F, T, int(t0), int(t1),
                      int(methods_mask), int(bool(average)), _lib.stream()))
    return out


def check_time_methods(method):
    """-> (list of names, whether a single name was given) for spectral_connectivity_time."""
    single = isinstance(method, str)
    names = [method] if single else list(method)
    if not names:
        raise ValueError("method is empty")
    for m in names:
        if m in CONTIME_MULTIVARIATE:
            raise NotImplementedError(f"method={m!r}: the multivariate and Granger measures are not provided; "
                                      f"provided: {', '.join(CONTIME_METHODS)}")
        if m not in CONTIME_METHODS:
            raise ValueError(f"method={m!r} (provided: {', '.join(CONTIME_METHODS)})")
    return names, single


def spectral_connectivity_time(data, freqs, method="coh", average=False, sfreq=None, faverage=False, bands=None,
                               padding=0.0, mode="cwt_morlet", n_cycles=7.0, decim=1, zero_mean=True, sm_times=0,
                               sm_freqs=1, indices=None):
    """Time-resolved connectivity of data [n, C, T] ([C, T] is n = 1) between every pair of channels, one map per
    trial -> (con, freqs): con real [n, F, C, C], or [F, C, C] with ``average=True`` (the mean over the trials of the
    per-trial measure, summed in fp64 in trial order on the device).

    With w_i(t) the complex Morlet coefficient of channel i at one frequency (``tfr_array_morlet(output='complex')``
    with these ``freqs``, ``n_cycles``, ``zero_mean`` and ``decim``), s = w_i conj(w_j), u = s / |s| (0 where
    |s| = 0) and <.> the mean over the kept samples of the trial:

        'coh'   |<s>| / sqrt(<|w_i|^2> <|w_j|^2>)          'pli'   |<sign Im s>|
        'imcoh' Im <s> / sqrt(<|w_i|^2> <|w_j|^2>)         'dpli'  <H(Im s)>, H(0) = 1/2
        'plv'   |<u>|                                      'wpli'  |<Im s>| / <|Im s|>
        'ciplv' |Im <u>| / sqrt((1 - |Re <u>|)(1 + |Re <u>|))
        'wpli2_debiased'  ((sum Im s)^2 - sum (Im s)^2) / ((sum |Im s|)^2 - sum (Im s)^2)

    ``method`` is one name or a list (a list returns a list; all entries share one pass over the map).  ``padding``
    (seconds) drops round(padding * sfreq / decim) output samples from each end before averaging; at least one must
    remain.  ``faverage=True`` averages each measure over the frequencies of each band of ``bands`` (default BANDS_5;
    both ends inclusive): con [..., n_bands, C, C] and freqs the bands' mean frequencies; a band without a frequency
    is an error.  Both triangles are filled: 'imcoh' and 'dpli' are antisymmetric (imcoh[j, i] = -imcoh[i, j],
    dpli[j, i] = 1 - dpli[i, j], exactly so in the output's arithmetic for i > j), the other six symmetric bit for bit.
    The diagonal is set, not computed: 1 for 'coh' and 'plv', 0 for 'imcoh' and 'pli', 1/2 for 'dpli' and NaN
    (0 / 0) for 'ciplv', 'wpli' and 'wpli2_debiased'.  A dead (all-zero) channel gives, off the diagonal of its row and
    column, NaN for 'coh', 'imcoh', 'wpli' and 'wpli2_debiased' (0 / 0), 0 for 'plv', 'ciplv' and 'pli' and 1/2 for
    'dpli'; no other entry changes.  The results are bitwise repeatable and do not depend on CONTIME_CHUNK_BYTES, the
    bound on the complex map alive at a time (trials are transformed and consumed in chunks).

    ndarray in -> the fp64 route -> float64 ndarray out; float32 / float64 CUDA tensor in -> a tensor of that dtype
    out, float32 with the transform and the products in fp32 and the sums in fp64 -- unless 'ciplv' is asked for: then
    the whole call runs the fp64 route and is rounded at the end (its denominator amplifies the rounding of <u>, as
    in ``spectral_connectivity``).  There is no CPU fallback.  Not provided (NotImplementedError): mode='multitaper',
    smoothing (``sm_times``, ``sm_freqs``), ``indices=``, the multivariate and Granger methods, more than MAX_CHANNELS
    channels.  Names and formulas follow mne-connectivity (``spectral_connectivity_time`` with no smoothing; 'dpli',
    'imcoh' and 'wpli2_debiased' as ``spectral_connectivity_epochs`` documents them, with time as the averaged axis);
    parity with that library is unpinned (it is not installed here)."""
    names, single = check_time_methods(method)
    if mode == "multitaper":
        raise NotImplementedError("mode='multitaper' is not provided: only 'cwt_morlet'")
    if mode != "cwt_morlet":
        raise ValueError(f"mode={mode!r} (need 'cwt_morlet')")
    if sm_times != 0 or sm_freqs != 1:
        raise NotImplementedError(f"sm_times={sm_times!r}, sm_freqs={sm_freqs!r}: smoothing of the cross-spectrum is "
                                  "not provided (need sm_times=0, sm_freqs=1)")
    if indices is not None:
        raise NotImplementedError("indices= is not provided: every pair of channels is computed")
    if sfreq is None:
        raise ValueError("sfreq is required")
    data, is_tensor = _lib.check_array(data, "data")
    if data.ndim not in (2, 3):
        raise ValueError(f"data must be [n, C, T] or [C, T], got {tuple(data.shape)}")
    if data.ndim == 2:
        data = data[None]
    n, Cc, T = (int(v) for v in data.shape)
    if not 1 <= Cc <= MAX_CHANNELS:
        raise NotImplementedError(f"{Cc} channels: 1 to {MAX_CHANNELS} are provided")
    decim = _tfr._check_decim(decim)
    sfreq, freqs, n_cycles = _tfr._freqs_cycles(sfreq, freqs, n_cycles)
    n_taps, taps_bytes = _tfr._cached_morlet(sfreq, freqs.tobytes(), n_cycles.tobytes(), bool(zero_mean))
    _tfr._check_taps(n_taps, T)
    padding = float(padding)
    if not padding >= 0:
        raise ValueError(f"padding={padding!r} (need >= 0 seconds)")
    T_out = _tfr.out_len(T, decim)
    t0 = int(round(padding * sfreq / decim))
    t1 = T_out - t0
    if t1 <= t0:
        raise ValueError(f"padding={padding:g} s drops {t0} of the {T_out} output samples from each end: none remains")
    if average and n == 0:
        raise ValueError("average=True over n=0 trials")
    F = int(freqs.size)
    out_freqs, bins = freqs.copy(), None
    if faverage:
        bands = BANDS_5 if bands is None else bands
        bins = band_bins(freqs, bands)
        for b, band in zip(bins, bands):
            if b.size == 0:
                raise ValueError(f"band {band!r} holds no frequency of freqs")
        out_freqs = np.array([freqs[b].mean() for b in bins])

    xd = _lib.to_device(data, is_tensor, "connectivity")
    out_dtype = xd.dtype
    if "ciplv" in names:
        xd = xd.double()
    f64 = xd.dtype == torch.float64
    order = sorted(set(names), key=CONTIME_METHODS.index)
    mask = contime_mask(order)
    plan = _tfr._cached_plan(n_taps, taps_bytes, decim, xd.device.index)
    per_trial = Cc * F * T_out * (16 if f64 else 8)
    step = max(1, min(max(n, 1), int(CONTIME_CHUNK_BYTES) // per_trial))
    zbuf = torch.empty((step, Cc, F, T_out), dtype=torch.complex128 if f64 else torch.complex64, device=xd.device)
    parts = []
    for s in range(0, n, step):
        c = min(step, n - s)
        z = plan(xd[s:s + c], "complex", out=zbuf[:c])
        part = contime_launch(z, mask, t0, t1, average=bool(average))
        parts.append(part.double() * c if average else part)
    if average:                                                   # chunk sums, added in chunk order in fp64
        res = parts[0]
        for p in parts[1:]:
            res = res + p
        res = (res / n).to(xd.dtype)
    elif parts:
        res = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
    else:
        res = torch.empty((len(order), 0, F, Cc, Cc), dtype=xd.dtype, device=xd.device)
    vals = [res[order.index(m)].to(out_dtype) for m in names]
    if faverage:
        vals = [_band_mean(v, bins) for v in vals]
    if not is_tensor:
        vals = [v.cpu().numpy() for v in vals]
    return (vals[0] if single else vals), out_freqs
