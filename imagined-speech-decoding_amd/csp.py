"""Common Spatial Patterns transformer of the classical baseline.

``CSP`` has the constructor surface of ``mne.decoding.CSP`` (argument order and defaults) and the sklearn transformer
protocol, so that the reference's ``Pipeline(CSP(8, log=True) -> StandardScaler -> SVC)``
(notebooks/svm_baseline.ipynb:240-248, :307, :316) takes it in place of MNE's, fed by ``filter_data``.  The two
data-sized steps run in libisd_hip.so (csrc/csp.hip): the per-trial covariances X Xᵀ / T with their per-class mean, and
the fused projection + average power (+ log) of ``transform``.  The decomposition of the [K, C, C] class covariances
is host work in float64 (``decompose``): a generalised eigen-decomposition for two classes, Pham's approximate joint
diagonalisation with mutual-information ordering (Grosse-Wentrup & Buss 2008) for more, restated from the published
method.  MNE is not vendored in the reference and is not installed here: parity is pinned against a NumPy restatement
(tests/test_csp_*.py), not against MNE.  There is no CPU fallback.  One CSP per band of a filterbank, on the raw
trials: ``isd_amd.FBCSP`` (fbcsp.py).
"""

import numpy as np
import torch

from . import _lib
from ._estimator import Estimator, cat_like, check_trials, chunks, transformer_tags

MAX_COMPONENTS = 16                  # isd_csp_power_*: 1 <= m <= 16
MAX_CHANNELS = 128                   # isd_trial_cov_*: 1 <= C <= 128
COV_CHUNK_BYTES = 256 << 20          # bound on the [chunk, C, C] covariance buffer of fit


def trial_covariances(x):
    """x CUDA tensor [n, C, T], float32 or float64 -> [n, C, C] of the same dtype: X_i X_iᵀ / T (no mean removal),
    exactly symmetric."""
    x = _lib.check_cuda(x, "x", MAX_CHANNELS)
    n, Cc, T = x.shape
    cov = torch.empty(n, Cc, Cc, dtype=x.dtype, device=x.device)
    if n:
        fn = _lib.typed("isd_trial_cov", x.dtype)
        with torch.cuda.device(x.device):
            _lib.check(fn(x.data_ptr(), cov.data_ptr(), n, Cc, T, _lib.stream()))
    return cov


def cov_group_mean(cov, idx, offs, norm_trace=False):
    """cov CUDA [n, C, C] (f32 / f64); idx int64 [offs[-1]] trial indices grouped by class; offs int64 [K + 1] ->
    CUDA float64 [K, C, C]: per-class mean (each trial divided by its trace first if ``norm_trace``), summed in fp64
    in the order of ``idx``."""
    if not (isinstance(cov, torch.Tensor) and cov.is_cuda and cov.dtype in (torch.float32, torch.float64)
            and cov.ndim == 3 and cov.shape[1] == cov.shape[2]):
        raise TypeError("cov must be a float32 or float64 CUDA tensor [n, C, C]")
    cov = cov.contiguous()
    idx_h = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
    offs_h = np.ascontiguousarray(offs, dtype=np.int64).reshape(-1)
    K = len(offs_h) - 1
    n = cov.shape[0]
    if K < 1 or offs_h[0] != 0 or np.any(np.diff(offs_h) < 0) or offs_h[-1] != len(idx_h):
        raise ValueError("offs must rise from 0 to len(idx)")
    if len(idx_h) and (idx_h.min() < 0 or idx_h.max() >= n):
        raise ValueError("idx out of range")
    idx_d = torch.as_tensor(idx_h).to(cov.device)
    offs_d = torch.as_tensor(offs_h).to(cov.device)
    out = torch.empty(K, cov.shape[1], cov.shape[1], dtype=torch.float64, device=cov.device)
    with torch.cuda.device(cov.device):
        _lib.check(_lib.lib().isd_cov_group_mean(cov.data_ptr(), int(cov.dtype == torch.float64), idx_d.data_ptr(),
                                                 offs_d.data_ptr(), int(bool(norm_trace)), out.data_ptr(), n,
                                                 cov.shape[1], K, _lib.stream()))
    return out


def csp_power(x, w, log=True):
    """x CUDA [n, C, T]; w [m, C] (1 <= m <= 16; tensor or array, cast to x's dtype) -> [n, m] of x's dtype:
    mean_t (w_j · x_i[:, t])², its log if ``log``.  The projected signal is never materialised."""
    x = _lib.check_cuda(x, "x", MAX_CHANNELS)
    n, Cc, T = x.shape
    w = torch.as_tensor(w).to(device=x.device, dtype=x.dtype).contiguous()
    if w.ndim != 2 or w.shape[1] != Cc or not 1 <= w.shape[0] <= MAX_COMPONENTS:
        raise ValueError(f"w must be [m, {Cc}] with 1 <= m <= {MAX_COMPONENTS}, got {tuple(w.shape)}")
    out = torch.empty(n, w.shape[0], dtype=x.dtype, device=x.device)
    if n:
        fn = _lib.typed("isd_csp_power", x.dtype)
        with torch.cuda.device(x.device):
            _lib.check(fn(x.data_ptr(), w.data_ptr(), out.data_ptr(), n, Cc, T, w.shape[0], int(bool(log)), _lib.stream()))
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


# ------------------------------------------------------------------------------------------- host decomposition
def _pham(covs, eps=1e-6, n_iter_max=15):
    """Pham's approximate joint diagonalisation of K real symmetric positive-definite matrices (D. T. Pham, 'Joint
    approximate diagonalization of positive definite Hermitian matrices', SIAM J. Matrix Anal. Appl. 2001).  Returns
    V [C, C] whose rows are the filters: V C_k Vᵀ is as diagonal as one non-orthogonal V can make all of them."""
    A = np.array(covs, dtype=np.float64)                         # [K, C, C], transformed in place
    K, Cc, _ = A.shape
    V = np.eye(Cc)
    for _ in range(n_iter_max):
        decrement = 0.0
        for i in range(1, Cc):
            for j in range(i):
                c1, c2, a = A[:, i, i], A[:, j, j], A[:, i, j]
                g12, g21 = np.mean(a / c1), np.mean(a / c2)
                w21, w12 = np.mean(c1 / c2), np.mean(c2 / c1)
                w = np.sqrt(w12 * w21)
                r = np.sqrt(w21 / w12)
                t1 = (r * g12 + g21) / (w + 1.0)
                t2 = (r * g12 - g21) / max(w - 1.0, 1e-9)
                h12, h21 = t1 + t2, (t1 - t2) / r
                decrement += K * (g12 * h12 + g21 * h21) / 2.0
                d = 1.0 + np.sqrt(1.0 - h12 * h21)
                tau = np.array([[1.0, -h12 / d], [-h21 / d, 1.0]])
                A[:, [i, j], :] = tau @ A[:, [i, j], :]
                A[:, :, [i, j]] = A[:, :, [i, j]] @ tau.T
                V[[i, j], :] = tau @ V[[i, j], :]
        if decrement < Cc * (Cc - 1) * eps:
            break
    return V


def decompose(covs, weights):
    """covs [K, C, C] class covariances, weights [K] per-class trial counts (host, float64) ->
    (filters [C, C], rows ordered most discriminative first; scores [C], non-increasing).

    K = 2: the generalised eigenvectors of (C_0, C_0 + C_1), ordered by |λ − 0.5| descending (scores = |λ − 0.5|).
    K > 2: Pham's joint diagonaliser, each filter v scaled to vᵀ C̄ v = 1 with C̄ the trial-count-weighted mean
    covariance, ordered by the mutual-information approximation of Grosse-Wentrup & Buss (2008),
    score = −(a + 3/16 b²), a = Σ_k p_k log √(vᵀ C_k v), b = Σ_k p_k ((vᵀ C_k v)² − 1), p_k the class frequency
    -- what MNE documents for component_order='mutual_info'.  Restated from the published method, not from MNE's
    code: parity with MNE itself is unpinned."""
    covs = np.asarray(covs, dtype=np.float64)
    weights = np.asarray(weights, dtype=np.float64).reshape(-1)
    if covs.ndim != 3 or covs.shape[1] != covs.shape[2]:
        raise ValueError(f"covs must be [K, C, C], got {covs.shape}")
    K = covs.shape[0]
    if K < 2:
        raise ValueError("CSP needs at least two classes")
    if len(weights) != K:
        raise ValueError(f"{len(weights)} weights for {K} classes")
    if K == 2:
        from scipy.linalg import eigh
        lam, vec = eigh(covs[0], covs.sum(0))
        scores = np.abs(lam - 0.5)
        order = np.argsort(-scores, kind="stable")
        return np.ascontiguousarray(vec.T[order]), scores[order]
    V = _pham(covs)
    p = weights / weights.sum()
    mean_cov = np.einsum("k,kab->ab", p, covs)
    V = V / np.sqrt(np.einsum("ia,ab,ib->i", V, mean_cov, V))[:, None]
    var = np.einsum("ia,kab,ib->ik", V, covs, V)                 # vᵀ C_k v, [C, K]
    a = (np.log(np.sqrt(var)) * p).sum(1)
    b = ((var ** 2 - 1.0) * p).sum(1)
    scores = -(a + 3.0 / 16.0 * b ** 2)
    order = np.argsort(-scores, kind="stable")
    return np.ascontiguousarray(V[order]), scores[order]


# --------------------------------------------------------------------------------------------------- estimator
class BandedCSP(Estimator):
    """The fit and transform that ``CSP`` and ``FBCSP`` share: one CSP per band of [n, C, T] trials, ``CSP`` being
    the case of one band.  A subclass sets ``_upload`` (the dtype an ndarray chunk is uploaded as; its size bounds the
    rows of a chunk), ``_dtypes`` (those of a tensor X) and ``_keep_bands`` (whether ``filters_``, ``scores_``,
    ``patterns_`` and ``covs_`` keep the leading band axis), extends ``_check_params`` and supplies

    ``_chunk_bytes()``           its module's COV_CHUNK_BYTES, read at call time;
    ``_start_fit(checked)``      called by fit once X and y have passed their checks, with what ``_check_params``
                                 returned; may store fitted state; -> n_bands;
    ``_chunk_covs(xc)``          xc CUDA [chunk, C, T] -> CUDA [chunk · n_bands, C, C], trial-major;
    ``_chunk_power(xc, w, log)`` w [n_bands, m, C] of dtype ``_upload`` -> CUDA, chunk · n_bands · m numbers in that
                                 order."""
    _upload, _dtypes, _keep_bands = np.float64, (torch.float32, torch.float64), False

    def __sklearn_tags__(self):
        return transformer_tags(required_y=True)

    def _check_params(self):
        if self.log is not None and not isinstance(self.log, (bool, np.bool_)):
            raise ValueError(f"log={self.log!r} (need None, True or False)")
        m = self.n_components
        if not isinstance(m, (int, np.integer)) or isinstance(m, bool) or m < 1:
            raise ValueError(f"n_components={m!r} (need a positive int)")
        if m > MAX_COMPONENTS:
            raise NotImplementedError(f"n_components={m}: at most {MAX_COMPONENTS} are provided")

    def _banded(self, a):
        """A fitted [n_bands, ...] array as the estimator publishes it: ``CSP`` drops the band axis."""
        return a if self._keep_bands else a[0]

    def _chunks(self, X, elements):
        """The chunks of X that keep a buffer of ``elements`` numbers a trial under ``_chunk_bytes()``."""
        rows = max(1, self._chunk_bytes() // (elements * np.dtype(self._upload).itemsize))
        return chunks(X, rows, type(self).__name__, self._upload)

    def _power(self, X, log):
        """[n, n_bands · m] average power of the picked components, band-major, in X's kind (ndarray -> float64
        ndarray)."""
        filters = self.filters_ if self._keep_bands else self.filters_[None]
        w = np.ascontiguousarray(filters[:, :self.n_components], dtype=self._upload)
        parts = [self._chunk_power(xc, w, log) for _, xc in self._chunks(X, X.shape[1] * X.shape[2])]
        return cat_like(parts, X, w.shape[:2]).reshape(X.shape[0], w.shape[0] * w.shape[1])

    def fit(self, X, y):
        """X [n, C, T] (ndarray, or CUDA tensor of one of ``_dtypes``), y [n] labels of at least two classes.
        Returns self."""
        checked = self._check_params()
        X = check_trials(X, self._dtypes)
        y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
        if y.ndim != 1 or len(y) != X.shape[0]:
            raise ValueError(f"X has {X.shape[0]} trials, y has shape {y.shape}")
        classes, yi = np.unique(y, return_inverse=True)
        K = len(classes)
        if K < 2:
            raise ValueError(f"{type(self).__name__} needs at least two classes")
        n, C_, T = X.shape
        if self.n_components > C_:
            raise ValueError(f"n_components={self.n_components} exceeds the {C_} channels")
        if C_ > MAX_CHANNELS:
            raise NotImplementedError(f"{C_} channels: at most {MAX_CHANNELS} are provided")
        if T < 1:
            raise ValueError("X has no samples")
        nb = self._start_fit(checked)
        counts = np.bincount(yi, minlength=K)
        # CSP's cov_est: with trials of equal length, 'concat' (covariance of the class's concatenated trials) and
        # 'epoch' (mean of the trial covariances) are the same number unless each trial is first divided by its trace
        covs = np.zeros((nb, K, C_, C_))
        for s, xc in self._chunks(X, nb * C_ * max(C_, T)):
            yc = yi[s:s + xc.shape[0]]
            idx, offs = band_major_groups(yc, K, nb)             # nb == 1: the chunk's trials sorted by class
            part = cov_group_mean(self._chunk_covs(xc), idx, offs, self.norm_trace).cpu().numpy()
            cnt = np.bincount(yc, minlength=K)
            covs += part.reshape(nb, K, C_, C_) * (cnt / counts)[None, :, None, None]     # chunks in order, fp64
        filters, scores = zip(*(decompose(covs[b], counts) for b in range(nb)))
        patterns = [np.linalg.pinv(f.T) for f in filters]
        self.classes_, self.covs_ = classes, self._banded(covs)
        self.filters_, self.scores_ = self._banded(np.stack(filters)), self._banded(np.stack(scores))
        self.patterns_ = self._banded(np.stack(patterns))
        self.n_channels_ = C_
        power = self._power(X, False)
        power = power.double().cpu().numpy() if isinstance(power, torch.Tensor) else power
        self.mean_, self.std_ = power.mean(0), power.std(0)
        return self

    def transform(self, X):
        """X [n, C, T] -> [n, n_bands · n_components]: log average power (``log`` None / True) or the z-scored
        average power ``(power − mean_) / std_`` (``log=False``)."""
        self._require_fitted("filters_", "fit(X, y) before transform")
        self._check_params()
        X = check_trials(X, self._dtypes)
        if X.shape[1] != self.n_channels_:
            raise ValueError(f"X has {X.shape[1]} channels, fit saw {self.n_channels_}")
        log = True if self.log is None else bool(self.log)
        power = self._power(X, log)
        if not log:
            if isinstance(power, torch.Tensor):
                power = (power - torch.as_tensor(self.mean_).to(power)) / torch.as_tensor(self.std_).to(power)
            else:
                power = (power - self.mean_) / self.std_
        return power

    def fit_transform(self, X, y=None, **fit_params):
        return self.fit(X, y).transform(X)


class CSP(BandedCSP):
    """Drop-in for ``mne.decoding.CSP`` inside an sklearn ``Pipeline`` (same argument order and defaults).
    ``log=None`` means True for 'average_power'.  ``reg``, ``rank``, ``cov_method_params``,
    ``transform_into='csp_space'``, another ``component_order`` and more than 16 components are not provided and
    raise NotImplementedError.  ndarray in -> fp64 on the GPU -> float64 ndarray [n, m] out; CUDA tensor in
    (f32 / f64) -> CUDA tensor of that dtype out."""
    _param_names = ("n_components", "reg", "log", "cov_est", "transform_into", "norm_trace", "cov_method_params",
                    "rank", "component_order")

    def __init__(self, n_components=4, reg=None, log=None, cov_est="concat", transform_into="average_power",
                 norm_trace=False, cov_method_params=None, rank=None, component_order="mutual_info"):
        self.n_components, self.reg, self.log, self.cov_est = n_components, reg, log, cov_est
        self.transform_into, self.norm_trace, self.cov_method_params = transform_into, norm_trace, cov_method_params
        self.rank, self.component_order = rank, component_order

    def _check_params(self):
        for name in ("reg", "rank", "cov_method_params"):
            if getattr(self, name) is not None:
                raise NotImplementedError(f"{name}={getattr(self, name)!r}: only None is provided")
        if self.transform_into != "average_power":
            if self.transform_into == "csp_space":
                raise NotImplementedError("transform_into='csp_space' is not provided")
            raise ValueError(f"transform_into={self.transform_into!r}")
        if self.component_order != "mutual_info":
            raise NotImplementedError(f"component_order={self.component_order!r}: only 'mutual_info' is provided")
        if self.cov_est not in ("concat", "epoch"):
            raise ValueError(f"cov_est={self.cov_est!r} (need 'concat' or 'epoch')")
        super()._check_params()

    def _chunk_bytes(self):
        return COV_CHUNK_BYTES

    def _start_fit(self, checked):
        return 1

    def _chunk_covs(self, xc):
        return trial_covariances(xc)

    def _chunk_power(self, xc, w, log):
        return csp_power(xc, w[0], log)
