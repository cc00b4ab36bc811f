"""Filter-bank Common Spatial Patterns (Ang, Chin, Zhang & Guan 2008): one CSP per band of a Butterworth filterbank,
the log-variance features of all bands side by side.

``FBCSP`` joins the two classical pieces of the package, the filterbank of ``extract_features`` and the ``CSP`` of
the SVM baseline, and takes the raw trials: ``Pipeline(FBCSP -> SelectKBest -> SVC)``.  The two data-sized steps run
in libisd_hip.so (csrc/fb.hip) on the filterbank plan's own cascade, without the filtered [n, n_bands, C, T] map in
memory: ``isd_fb_trial_cov`` filters a trial's channels and feeds the matrix cores from LDS (fit), and
``isd_fb_csp_power`` projects first and filters the ``n_components`` projected rows instead of the C channels
(transform; filter and projection commute).  Fit and transform themselves are ``csp.BandedCSP``, which ``CSP`` runs
with one band: the per-(band, class) mean is ``csp.cov_group_mean`` and the decomposition ``csp.decompose``.  The data
path is fp32 (bands that ``precision='auto'`` sends to fp64 run their recursion in fp64; the covariance product, the
projection and the power sum are fp32).  Feature selection is sklearn's, like the scaler and the SVC.  Not provided:
zero-phase or Chebyshev banks, a gradient, ``reg`` / shrinkage, an fp64 data path.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import _lib
from .constants import BANDS_9, band_edges
from .csp import MAX_CHANNELS, MAX_COMPONENTS, BandedCSP, band_major_groups  # noqa: F401  (a re-export)
from .features import Filterbank

COV_CHUNK_BYTES = 256 << 20          # bound on the [chunk, n_bands, C, C] covariance buffer of fit


def fb_trial_covariances(x, fb):
    """x CUDA float32 [n, C, T], fb a ``features.Filterbank`` -> CUDA float32 [n, n_bands, C, C]: Y Yᵀ / T of every
    band's causally filtered trial Y (zero initial state, no mean removal), exactly symmetric."""
    x = _lib.check_cuda(x, "x", MAX_CHANNELS, (torch.float32,))
    if not isinstance(fb, Filterbank):
        raise TypeError("fb must be a features.Filterbank")
    n, Cc, T = x.shape
    cov = torch.empty(n, fb.n_bands, Cc, Cc, dtype=torch.float32, device=x.device)
    if n:
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().isd_fb_trial_cov(fb._h, x.data_ptr(), cov.data_ptr(), n, Cc, T, _lib.stream()))
    return cov


def fb_csp_power(x, fb, w, log=True):
    """x CUDA float32 [n, C, T]; w [n_bands, m, C] (1 <= m <= 16; tensor or array, cast to float32) -> CUDA float32
    [n, n_bands, m]: the mean over time of the squared band-b output of the projected row w[b, j] · x_i, its log if
    ``log``.  The projection is formed first and then filtered."""
    x = _lib.check_cuda(x, "x", MAX_CHANNELS, (torch.float32,))
    if not isinstance(fb, Filterbank):
        raise TypeError("fb must be a features.Filterbank")
    n, Cc, T = x.shape
    w = torch.as_tensor(w).to(device=x.device, dtype=torch.float32).contiguous()
    if w.ndim != 3 or w.shape[0] != fb.n_bands or w.shape[2] != Cc or not 1 <= w.shape[1] <= MAX_COMPONENTS:
        raise ValueError(f"w must be [{fb.n_bands}, m, {Cc}] with 1 <= m <= {MAX_COMPONENTS}, got {tuple(w.shape)}")
    m = w.shape[1]
    out = torch.empty(n, fb.n_bands, m, dtype=torch.float32, device=x.device)
    if n:
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().isd_fb_csp_power(fb._h, x.data_ptr(), w.data_ptr(), out.data_ptr(), n, Cc, T, m,
                                                   int(bool(log)), _lib.stream()))
    return out


class FBCSP(BandedCSP):
    """Filter-bank CSP transformer with the sklearn protocol of ``CSP``: ``fit(X, y)`` learns one CSP per band,
    ``transform(X)`` returns [n, n_bands · n_components] with feature b · n_components + j the (log) average power of
    component j of band b.  ``log=None`` means True; ``log=False`` returns the z-scored power ``(power − mean_) /
    std_``.  ``precision`` is the filterbank's ('auto', 'f32', 'f64': the arithmetic of the recursion).

    ndarray in (any float dtype, uploaded chunk by chunk as float32) -> float64 ndarray out; CUDA float32 tensor in ->
    CUDA float32 tensor out.  The arithmetic is fp32 either way.  More than 16 components or 128 channels raise
    NotImplementedError."""
    _param_names = ("n_components", "bands", "sfreq", "order", "log", "norm_trace", "precision")
    _upload, _dtypes, _keep_bands = np.float32, (torch.float32,), True

    def __init__(self, n_components=4, bands=BANDS_9, sfreq=250.0, order=4, log=None, norm_trace=False,
                 precision="auto"):
        self.n_components, self.bands, self.sfreq, self.order = n_components, bands, sfreq, order
        self.log, self.norm_trace, self.precision = log, norm_trace, precision

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_fb", None)                                   # a library handle; rebuilt on demand
        return state

    def _check_params(self):
        """-> the (lo, hi) edges of the bands"""
        super()._check_params()
        if self.precision not in ("auto", "f32", "f64"):
            raise ValueError(f"precision={self.precision!r} (need 'auto', 'f32' or 'f64')")
        if not isinstance(self.order, (int, np.integer)) or isinstance(self.order, bool) or not 1 <= self.order <= 8:
            raise ValueError(f"order={self.order!r} (need an int in 1 .. 8)")
        if not float(self.sfreq) > 0:
            raise ValueError(f"sfreq={self.sfreq!r}")
        edges = band_edges(self.bands)
        if not edges:
            raise ValueError("bands is empty")
        for lo, hi in edges:
            if not 0.0 < lo < hi < float(self.sfreq) / 2:
                raise ValueError(f"band ({lo}, {hi}) Hz is not inside (0, sfreq / 2) = (0, {float(self.sfreq) / 2})")
        return edges

    def _filterbank(self):
        key = (tuple(self.bands_), float(self.sfreq), int(self.order), self.precision)
        if getattr(self, "_fb", None) is None or self._fb[0] != key:
            self._fb = (key, Filterbank([("b", lo, hi) for lo, hi in self.bands_], float(self.sfreq), int(self.order),
                                        self.precision))
        return self._fb[1]

    def _chunk_bytes(self):
        return COV_CHUNK_BYTES

    def _start_fit(self, edges):
        self.bands_ = edges
        return len(edges)

    def _chunk_covs(self, xc):
        return fb_trial_covariances(xc, self._filterbank()).view(-1, xc.shape[1], xc.shape[1])

    def _chunk_power(self, xc, w, log):
        return fb_csp_power(xc, self._filterbank(), w, log)
