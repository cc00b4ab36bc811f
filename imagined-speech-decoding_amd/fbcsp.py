"""Filter-bank Common Spatial Patterns (Ang, Chin, Zhang & Guan 2008): one CSP per band of a Butterworth filterbank,
the log-variance features of all bands side by side.

``FBCSP`` joins the two classical pieces of the package, the filterbank of ``extract_features`` and the ``CSP`` of
the SVM baseline, and takes the raw trials: ``Pipeline(FBCSP -> SelectKBest -> SVC)``.  The two data-sized steps run
in libisd_hip.so (csrc/fb.hip) on the filterbank plan's own cascade, without the filtered [n, n_bands, C, T] map in
memory: ``isd_fb_trial_cov`` filters a trial's channels and feeds the matrix cores from LDS (fit), and
``isd_fb_csp_power`` projects first and filters the ``n_components`` projected rows instead of the C channels
(transform; filter and projection commute).  The per-(band, class) mean is ``csp.cov_group_mean`` and the
decomposition ``csp.decompose``, unchanged.  The data path is fp32 (bands that ``precision='auto'`` sends to fp64 run
their recursion in fp64; the covariance product, the projection and the power sum are fp32).  Feature selection is
sklearn's, like the scaler and the SVC.  Not provided: zero-phase or Chebyshev banks, a gradient, ``reg`` / shrinkage,
an fp64 data path.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import _lib, csp
from .classifier import NotFittedError
from .constants import BANDS_9, band_edges
from .csp import MAX_CHANNELS, MAX_COMPONENTS
from .features import Filterbank

COV_CHUNK_BYTES = 256 << 20          # bound on the [chunk, n_bands, C, C] covariance buffer of fit


def _check_x(x):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
        raise TypeError("x must be a float32 CUDA tensor")
    if x.ndim != 3:
        raise ValueError(f"x must be [n, C, T], got {tuple(x.shape)}")
    if not 1 <= x.shape[1] <= MAX_CHANNELS or x.shape[2] < 1:
        raise ValueError(f"x [n, C, T] needs 1 <= C <= {MAX_CHANNELS} and T >= 1, got {tuple(x.shape)}")
    return x.contiguous()


def fb_trial_covariances(x, fb):
    """x CUDA float32 [n, C, T], fb a ``features.Filterbank`` -> CUDA float32 [n, n_bands, C, C]: Y Yᵀ / T of every
    band's causally filtered trial Y (zero initial state, no mean removal), exactly symmetric."""
    x = _check_x(x)
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
    x = _check_x(x)
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


def band_major_groups(yc, K, nb):
    """Group index of a chunk for ``cov_group_mean`` on the [chunk · nb, C, C] view of its [chunk, nb, C, C]
    covariances.  yc [chunk] class indices in [0, K) -> (idx, offs): group b · K + k lists the rows i · nb + b of the
    chunk's trials i of class k, in trial order; offs [nb · K + 1]."""
    yc = np.asarray(yc, dtype=np.int64).reshape(-1)
    order = np.argsort(yc, kind="stable")                        # the chunk's trials sorted by class
    cnt = np.bincount(yc, minlength=K)
    idx = (order[None, :] * nb + np.arange(nb, dtype=np.int64)[:, None]).reshape(-1)
    offs = np.concatenate([[0], np.cumsum(np.tile(cnt, nb))]).astype(np.int64)
    return idx, offs


class FBCSP:
    """Filter-bank CSP transformer with the sklearn protocol of ``CSP``: ``fit(X, y)`` learns one CSP per band,
    ``transform(X)`` returns [n, n_bands · n_components] with feature b · n_components + j the (log) average power of
    component j of band b.  ``log=None`` means True; ``log=False`` returns the z-scored power ``(power − mean_) /
    std_``.  ``precision`` is the filterbank's ('auto', 'f32', 'f64': the arithmetic of the recursion).

    ndarray in (any float dtype, uploaded chunk by chunk as float32) -> float64 ndarray out; CUDA float32 tensor in ->
    CUDA float32 tensor out.  The arithmetic is fp32 either way.  More than 16 components or 128 channels raise
    NotImplementedError."""
    _param_names = ("n_components", "bands", "sfreq", "order", "log", "norm_trace", "precision")

    def __init__(self, n_components=4, bands=BANDS_9, sfreq=250.0, order=4, log=None, norm_trace=False,
                 precision="auto"):
        self.n_components, self.bands, self.sfreq, self.order = n_components, bands, sfreq, order
        self.log, self.norm_trace, self.precision = log, norm_trace, precision

    def get_params(self, deep=True):
        return {k: getattr(self, k) for k in self._param_names}

    def set_params(self, **params):
        for k, v in params.items():
            if k not in self._param_names:
                raise ValueError(f"invalid parameter {k!r} for {type(self).__name__}")
            setattr(self, k, v)
        return self

    def __sklearn_tags__(self):
        """Called by sklearn only (Pipeline, clone, checks), so sklearn is imported here and nowhere else."""
        from sklearn.utils import InputTags, Tags, TargetTags, TransformerTags
        return Tags(estimator_type=None, target_tags=TargetTags(required=True), transformer_tags=TransformerTags(),
                    input_tags=InputTags(three_d_array=True))

    def __repr__(self):
        return f"FBCSP({', '.join(f'{k}={getattr(self, k)!r}' for k in self._param_names)})"

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_fb", None)                                   # a library handle; rebuilt on demand
        return state

    def _check_params(self):
        m = self.n_components
        if not isinstance(m, (int, np.integer)) or isinstance(m, bool) or m < 1:
            raise ValueError(f"n_components={m!r} (need a positive int)")
        if m > MAX_COMPONENTS:
            raise NotImplementedError(f"n_components={m}: at most {MAX_COMPONENTS} are provided")
        if self.log is not None and not isinstance(self.log, (bool, np.bool_)):
            raise ValueError(f"log={self.log!r} (need None, True or False)")
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

    @staticmethod
    def _check_X(X):
        if isinstance(X, torch.Tensor) and X.is_cuda and X.dtype != torch.float32:
            raise TypeError("a tensor X must be float32 (the data path is fp32)")
        X, _ = _lib.check_array(X, "X", (torch.float32,))
        if X.ndim != 3:
            raise ValueError(f"X must be [n, C, T], got {tuple(X.shape)}")
        return X

    @staticmethod
    def _chunks(X, rows):
        """CUDA float32 [<= rows, C, T] slices of X in order; an ndarray is uploaded slice by slice."""
        is_tensor = isinstance(X, torch.Tensor)
        for s in range(0, X.shape[0], rows):
            yield s, _lib.to_device(X[s:s + rows], is_tensor, "FBCSP", np.float32)

    def _filterbank(self):
        key = (tuple(self.bands_), float(self.sfreq), int(self.order), self.precision)
        if getattr(self, "_fb", None) is None or self._fb[0] != key:
            self._fb = (key, Filterbank([("b", lo, hi) for lo, hi in self.bands_], float(self.sfreq), int(self.order),
                                        self.precision))
        return self._fb[1]

    def _power(self, X, log):
        """[n, nb, m] average power of the picked components, in X's kind (ndarray -> float64 ndarray)."""
        C_, T = X.shape[1], X.shape[2]
        nb, m = len(self.bands_), self.n_components
        rows = max(1, COV_CHUNK_BYTES // (C_ * T * 4))
        fb = self._filterbank()
        w = np.ascontiguousarray(self.filters_[:, :m], dtype=np.float32)
        parts = [fb_csp_power(xc, fb, w, log) for _, xc in self._chunks(X, rows)]
        if isinstance(X, torch.Tensor):
            return torch.cat(parts) if parts else torch.empty(0, nb, m, dtype=torch.float32, device=X.device)
        return torch.cat(parts).double().cpu().numpy() if parts else np.empty((0, nb, m))

    def fit(self, X, y):
        """X [n, C, T] (float ndarray, or float32 CUDA tensor) of raw trials, y [n] labels of at least two classes.
        Returns self."""
        edges = self._check_params()
        X = self._check_X(X)
        y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
        if y.ndim != 1 or len(y) != X.shape[0]:
            raise ValueError(f"X has {X.shape[0]} trials, y has shape {y.shape}")
        classes, yi = np.unique(y, return_inverse=True)
        K = len(classes)
        if K < 2:
            raise ValueError("FBCSP needs at least two classes")
        n, C_, T = X.shape
        if C_ > MAX_CHANNELS:
            raise NotImplementedError(f"{C_} channels: at most {MAX_CHANNELS} are provided")
        if self.n_components > C_:
            raise ValueError(f"n_components={self.n_components} exceeds the {C_} channels")
        if T < 1:
            raise ValueError("X has no samples")
        nb = len(edges)
        self.bands_ = edges
        fb = self._filterbank()
        counts = np.bincount(yi, minlength=K)
        covs = np.zeros((nb, K, C_, C_))
        rows = max(1, COV_CHUNK_BYTES // (nb * C_ * max(C_, T) * 4))
        for s, xc in self._chunks(X, rows):
            yc = yi[s:s + xc.shape[0]]
            idx, offs = band_major_groups(yc, K, nb)
            cov = fb_trial_covariances(xc, fb).view(-1, C_, C_)
            part = csp.cov_group_mean(cov, idx, offs, self.norm_trace).cpu().numpy().reshape(nb, K, C_, C_)
            covs += part * (np.bincount(yc, minlength=K) / counts)[None, :, None, None]   # chunks in order, fp64
        filters, scores = zip(*(csp.decompose(covs[b], counts) for b in range(nb)))
        self.classes_, self.covs_ = classes, covs
        self.filters_, self.scores_ = np.stack(filters), np.stack(scores)
        self.patterns_ = np.stack([np.linalg.pinv(f.T) for f in filters])
        self.n_channels_ = C_
        power = self._power(X, False)
        power = power.double().cpu().numpy() if isinstance(power, torch.Tensor) else power
        power = power.reshape(n, -1)
        self.mean_, self.std_ = power.mean(0), power.std(0)
        return self

    def transform(self, X):
        """X [n, C, T] -> [n, n_bands · n_components]: log average power (``log`` None / True) or the z-scored
        average power ``(power − mean_) / std_`` (``log=False``)."""
        if not hasattr(self, "filters_"):
            raise NotFittedError("this FBCSP instance is not fitted yet: call fit(X, y) before transform")
        self._check_params()
        X = self._check_X(X)
        if X.shape[1] != self.n_channels_:
            raise ValueError(f"X has {X.shape[1]} channels, fit saw {self.n_channels_}")
        log = True if self.log is None else bool(self.log)
        power = self._power(X, log)
        power = power.reshape(power.shape[0], -1)
        if not log:
            if isinstance(power, torch.Tensor):
                power = (power - torch.as_tensor(self.mean_).to(power)) / torch.as_tensor(self.std_).to(power)
            else:
                power = (power - self.mean_) / self.std_
        return power

    def fit_transform(self, X, y=None, **fit_params):
        return self.fit(X, y).transform(X)
