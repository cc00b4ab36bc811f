"""Riemannian geometry of covariance matrices: the covariance-manifold baseline beside CSP + SVM.

``Covariances -> TangentSpace -> LogisticRegression / SVC`` and ``Covariances -> MDM`` (minimum distance to the Riemannian
mean; Barachant, Bonnet, Congedo & Jutten 2012), with pyriemann's argument names and defaults and the sklearn protocol,
so that either drops into the ``Pipeline`` of notebooks/svm_baseline.ipynb in place of ``CSP -> StandardScaler``.
The data-sized steps run in libisd_hip.so (csrc/riemann.hip) in float64: the congruence W C_i Wᵀ of every trial
covariance on the fp64 matrix cores, and the matrix function (log, sqrt, ...) of n small symmetric positive-definite
matrices by a batched one-sided Jacobi eigen-decomposition.  What works on the [K, C, C] class means (their square
roots, exp, the step control of the mean iteration) is host work in float64 with NumPy ``eigh``, as ``csp.decompose``.
pyriemann is not vendored in the reference and is not installed here: the behaviour is restated from the published
method and pinned against a NumPy restatement (tests/riemann_ref.py); parity with pyriemann itself is unpinned.
``CoSpectra`` gives one SPD matrix per trial and frequency (the real part of ``connectivity.csd_array_welch``) for a
tangent space per frequency.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import _lib
from ._estimator import Estimator, cat_like, check_trials, chunks, like, transformer_tags
from .csp import COV_CHUNK_BYTES, MAX_CHANNELS, cov_group_mean, trial_covariances

SPD_LOG, SPD_SQRT, SPD_INVSQRT, SPD_INV, SPD_NONE = range(5)     # ISD_SPD_* of include/isd_hip.h
SPD_FULL, SPD_TANGENT, SPD_NOOUT = range(3)
_FN = {"log": SPD_LOG, "sqrt": SPD_SQRT, "invsqrt": SPD_INVSQRT, "inv": SPD_INV, "none": SPD_NONE}
_OUT = {"full": SPD_FULL, "tangent": SPD_TANGENT}


# ----------------------------------------------------------------------------------------------------- low level
def _device_stack(a, name="covs"):
    """[n, C, C] ndarray (uploaded as float64) or CUDA tensor -> checked contiguous CUDA tensor."""
    a, is_tensor = _lib.check_array(a, name)
    if a.ndim != 3 or a.shape[1] != a.shape[2]:
        raise ValueError(f"{name} must be [n, C, C], got {tuple(a.shape)}")
    return _lib.check_cuda(_lib.to_device(a, is_tensor, "riemann"), name, MAX_CHANNELS, square=True)


def congruence(cov, W, widx=None):
    """cov CUDA [n, C, C] (f32 / f64); W [K, C, C] or [C, C] (tensor or array, used as float64); widx [n] ints in
    [0, K) or None (then W[0] for every matrix) -> CUDA float64 [n, C, C]: W_k cov_i W_kᵀ, exactly symmetric."""
    cov = _lib.check_cuda(cov, "cov", MAX_CHANNELS, square=True)
    n, Cc, _ = cov.shape
    W = torch.as_tensor(W).to(device=cov.device, dtype=torch.float64)
    if W.ndim == 2:
        W = W[None]
    if W.ndim != 3 or W.shape[0] < 1 or tuple(W.shape[1:]) != (Cc, Cc):
        raise ValueError(f"W must be [K, {Cc}, {Cc}], got {tuple(W.shape)}")
    W = W.contiguous()
    K = W.shape[0]
    idx_ptr = None
    if widx is not None:
        idx_h = np.asarray(widx.detach().cpu() if isinstance(widx, torch.Tensor) else widx).reshape(-1)
        if len(idx_h) != n:
            raise ValueError(f"widx has {len(idx_h)} entries for {n} matrices")
        if n and (idx_h.min() < 0 or idx_h.max() >= K):
            raise ValueError(f"widx outside [0, {K})")
        idx_d = torch.as_tensor(np.ascontiguousarray(idx_h, dtype=np.int32)).to(cov.device)
        idx_ptr = idx_d.data_ptr()
    out = torch.empty(n, Cc, Cc, dtype=torch.float64, device=cov.device)
    if n:
        with torch.cuda.device(cov.device):
            _lib.check(_lib.lib().isd_spd_congruence(cov.data_ptr(), int(cov.dtype == torch.float64), W.data_ptr(),
                                                     idx_ptr, out.data_ptr(), n, Cc, K, _lib.stream()))
    return out


def _eigfun(a, fn, out_kind, want_eigvals):
    """a CUDA float64 [n, C, C] -> (out or None, eigvals or None, info int32 [n]); no check of info."""
    n, Cc, _ = a.shape
    out = eig = None
    if out_kind == SPD_FULL:
        out = torch.empty(n, Cc, Cc, dtype=torch.float64, device=a.device)
    elif out_kind == SPD_TANGENT:
        out = torch.empty(n, Cc * (Cc + 1) // 2, dtype=torch.float64, device=a.device)
    if want_eigvals:
        eig = torch.empty(n, Cc, dtype=torch.float64, device=a.device)
    info = torch.zeros(n, dtype=torch.int32, device=a.device)
    if n:
        with torch.cuda.device(a.device):
            _lib.check(_lib.lib().isd_spd_eigfun(a.data_ptr(), None if out is None else out.data_ptr(),
                                                 None if eig is None else eig.data_ptr(), info.data_ptr(), n, Cc, fn,
                                                 out_kind, _lib.stream()))
    return out, eig, info


def _raise_on_failure(info):
    bad = torch.nonzero(info <= 0).reshape(-1)
    if bad.numel():
        i = int(bad[0])
        code = int(info[i])
        why = "the Jacobi iteration did not converge in 30 sweeps" if code == -1 else \
            "it is not symmetric positive definite (an eigenvalue is <= 0 or not finite)"
        raise ValueError(f"matrix {i} of the batch: {why} ({bad.numel()} of {info.numel()} matrices failed)")


def spd_function(a, fn, out="full", return_info=False):
    """f(A_i) = V f(Λ) Vᵀ of every symmetric positive-definite matrix of a CUDA [n, C, C] stack (f32 / f64 in,
    float64 arithmetic and result).  ``fn``: 'log', 'sqrt', 'invsqrt', 'inv' or 'none'.  ``out='full'`` -> [n, C, C],
    exactly symmetric; ``out='tangent'`` -> [n, C (C + 1) / 2], the upper triangle in ``np.triu_indices(C)`` order with
    the off-diagonal entries times √2.  A matrix that fails (not positive definite, not finite, no convergence) raises
    ValueError naming its index; with ``return_info`` nothing is raised and (result, info int32 [n]) is returned:
    sweeps used (> 0), -1 sweep cap reached, -2 bad eigenvalue (that matrix's result is NaN)."""
    if fn not in _FN:
        raise ValueError(f"fn={fn!r} (need one of {sorted(_FN)})")
    if out not in _OUT:
        raise ValueError(f"out={out!r} (need 'full' or 'tangent')")
    a = _lib.check_cuda(a, "a", MAX_CHANNELS, square=True).double()
    res, _, info = _eigfun(a, _FN[fn], _OUT[out], False)
    if return_info:
        return res, info
    _raise_on_failure(info)
    return res


def spd_eigvalsh(a):
    """Eigenvalues of every matrix of a CUDA [n, C, C] stack of symmetric positive semi-definite matrices ->
    CUDA float64 [n, C], ascending."""
    a = _lib.check_cuda(a, "a", MAX_CHANNELS, square=True).double()
    _, eig, info = _eigfun(a, SPD_NONE, SPD_NOOUT, True)
    _raise_on_failure(info)
    return torch.sort(eig, dim=1).values


# ------------------------------------------------------------------------------------------ host [K, C, C] work
def _host_fun(M, f):
    """f(M) of one symmetric host matrix through NumPy eigh, symmetrised."""
    lam, V = np.linalg.eigh(M)
    out = (V * f(lam)) @ V.T
    return (out + out.T) / 2


def _host_spd(M, name):
    M = np.asarray(M.detach().cpu() if isinstance(M, torch.Tensor) else M, dtype=np.float64)
    if M.ndim == 2:
        M = M[None]
    if M.ndim != 3 or M.shape[1] != M.shape[2]:
        raise ValueError(f"{name} must be [C, C] or [K, C, C], got {M.shape}")
    return M


def _invsqrt_checked(M, name):
    out = np.empty_like(M)
    for k, Mk in enumerate(M):
        lam = np.linalg.eigvalsh(Mk) if np.all(np.isfinite(Mk)) else np.array([np.nan])
        if not (np.all(np.isfinite(lam)) and lam.min() > 0):
            raise ValueError(f"{name}[{k}] is not symmetric positive definite")
        out[k] = _host_fun(Mk, lambda v: v ** -0.5)
    return out


# --------------------------------------------------------------------------------------------------- functions
def tangent_space(covs, Cref):
    """covs [n, C, C] (ndarray or CUDA tensor), Cref [C, C] -> CUDA float64 [n, C (C + 1) / 2]: the tangent vectors
    upper(log(Cref^-1/2 C_i Cref^-1/2)) with off-diagonal entries times √2, so that the Euclidean norm of a row is the
    Riemannian distance of C_i to Cref."""
    covs = _device_stack(covs)
    W = _invsqrt_checked(_host_spd(Cref, "Cref"), "Cref")
    if W.shape[0] != 1 or W.shape[1] != covs.shape[1]:
        raise ValueError(f"Cref must be [{covs.shape[1]}, {covs.shape[1]}], got {W.shape[1:]}")
    out, _, info = _eigfun(congruence(covs, W), SPD_LOG, SPD_TANGENT, False)
    _raise_on_failure(info)
    return out


def distance_riemann(A, B):
    """Affine-invariant distance √Σ log² λ(B^-1/2 A B^-1/2).  A [n, C, C] (ndarray or CUDA tensor); B [C, C] ->
    CUDA float64 [n], or B [K, C, C] -> [n, K]."""
    A = _device_stack(A, "A")
    single = (B.ndim if isinstance(B, (torch.Tensor, np.ndarray)) else np.ndim(B)) == 2
    W = _invsqrt_checked(_host_spd(B, "B"), "B")
    if W.shape[1] != A.shape[1]:
        raise ValueError(f"B has {W.shape[1]} channels, A has {A.shape[1]}")
    cols = []
    for k in range(W.shape[0]):
        _, eig, info = _eigfun(congruence(A, W[k]), SPD_LOG, SPD_NOOUT, True)
        _raise_on_failure(info)
        cols.append(torch.log(eig).square().sum(1).sqrt())
    return cols[0] if single else torch.stack(cols, dim=1)


def mean_riemann(covs, tol=1e-8, maxiter=50, init=None, sample_weight=None, groups=None, return_n_iter=False):
    """Riemannian (Karcher) mean of SPD matrices by the fixed-point iteration with adaptive step
    (Fletcher & Joshi 2004 as used by Barachant et al.).  covs [n, C, C] ndarray or CUDA tensor.

    From M = the (weighted) arithmetic mean, or ``init``:  J = Σ w_i log(M^-1/2 C_i M^-1/2),
    M <- M^1/2 exp(ν J) M^1/2,  crit = ‖J‖_F,  h = ν crit;  h < τ: ν <- 0.95 ν, τ <- h;  else ν <- 0.5 ν;  until
    crit <= tol, ν <= tol or ``maxiter`` iterations (ν = 1 and τ = the largest float at the start; w sums to 1).

    ``groups`` [n] integer labels: the mean of every group, [K, C, C] in the order of ``np.unique(groups)``; all
    groups advance in one pass over the trials per iteration, a group that has converged stops moving, and each
    group's result is bit for bit that of a call on its matrices alone.  ``init`` is then [K, C, C].
    Returns a float64 ndarray [C, C] ([K, C, C] with groups); with ``return_n_iter`` also the iteration count (an
    int, or an int array [K])."""
    covs = _device_stack(covs)
    n, Cc, _ = covs.shape
    if n < 1:
        raise ValueError("mean_riemann needs at least one matrix")
    if groups is None:
        gi, K = np.zeros(n, dtype=np.int64), 1
    else:
        g = np.asarray(groups.detach().cpu() if isinstance(groups, torch.Tensor) else groups)
        if g.shape != (n,):
            raise ValueError(f"groups must be [{n}], got {g.shape}")
        gi = np.unique(g, return_inverse=True)[1].reshape(-1)
        K = int(gi.max()) + 1
    counts = np.bincount(gi, minlength=K)
    idx = np.argsort(gi, kind="stable")                          # the trials grouped, in their own order
    offs = np.concatenate([[0], np.cumsum(counts)])
    scale = None
    if sample_weight is not None:
        w = np.asarray(sample_weight, dtype=np.float64).reshape(-1)
        if w.shape != (n,) or not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError(f"sample_weight must be [{n}], finite and non-negative")
        tot = np.array([w[idx[offs[k]:offs[k + 1]]].sum() for k in range(K)])   # summed in each group's own order
        if np.any(tot <= 0):
            raise ValueError("a group's weights sum to zero")
        # the group mean divides by the count: w_i / tot_k = scale_i / count_k
        scale = torch.as_tensor(w / tot[gi] * counts[gi]).to(covs.device)[:, None, None]

    def weighted_mean(stack):
        return cov_group_mean(stack if scale is None else stack.double() * scale, idx, offs).cpu().numpy()

    if init is None:
        M = weighted_mean(covs)
        M = (M + M.transpose(0, 2, 1)) / 2
    else:
        M = _host_spd(init, "init").copy()
        if M.shape != (K, Cc, Cc):
            raise ValueError(f"init must be [{K}, {Cc}, {Cc}]" if groups is not None else f"init must be [{Cc}, {Cc}]")
    nu = np.ones(K)
    tau = np.full(K, np.finfo(np.float64).max)
    crit = np.full(K, np.finfo(np.float64).max)
    n_iter = np.zeros(K, dtype=np.int64)
    active = np.ones(K, dtype=bool)
    W = np.tile(np.eye(Cc), (K, 1, 1))
    half = W.copy()
    for _ in range(int(maxiter)):
        active &= (crit > tol) & (nu > tol)
        if not active.any():
            break
        for k in np.flatnonzero(active):
            lam, V = np.linalg.eigh(M[k])
            if not (np.all(np.isfinite(lam)) and lam.min() > 0):
                raise ValueError(f"the mean of group {k} left the positive-definite cone")
            W[k] = (V * lam ** -0.5) @ V.T
            half[k] = (V * lam ** 0.5) @ V.T
        logs, _, info = _eigfun(congruence(covs, W, gi if K > 1 else None), SPD_LOG, SPD_FULL, False)
        _raise_on_failure(info)
        J = weighted_mean(logs)
        for k in np.flatnonzero(active):
            Jk = (J[k] + J[k].T) / 2
            Mk = half[k] @ _host_fun(nu[k] * Jk, np.exp) @ half[k]
            M[k] = (Mk + Mk.T) / 2
            n_iter[k] += 1
            crit[k] = np.linalg.norm(Jk)
            h = nu[k] * crit[k]
            if h < tau[k]:
                nu[k], tau[k] = 0.95 * nu[k], h
            else:
                nu[k] = 0.5 * nu[k]
    out = M if groups is not None else M[0]
    if return_n_iter:
        return out, (n_iter if groups is not None else int(n_iter[0]))
    return out


# --------------------------------------------------------------------------------------------------- estimators
class _Estimator(Estimator):
    """What the estimators on [n, C, C] covariance stacks share beyond the protocol of ``Estimator``."""

    def _fitted(self, attr):
        self._require_fitted(attr, "fit before using it")

    @staticmethod
    def _check_covs(X):
        """[n, C, C] ndarray or CUDA f32 / f64 tensor, checked but not moved."""
        X, _ = _lib.check_array(X, "X")
        if X.ndim != 3 or X.shape[1] != X.shape[2]:
            raise ValueError(f"X must be [n, C, C], got {tuple(X.shape)}")
        if X.shape[1] > MAX_CHANNELS:
            raise NotImplementedError(f"{X.shape[1]} channels: at most {MAX_CHANNELS} are provided")
        return X


class Covariances(_Estimator):
    """Drop-in for ``pyriemann.estimation.Covariances``: X [n, C, T] -> [n, C, C].  ``estimator='scm'`` is the sample
    covariance X Xᵀ / T without mean removal (``isd_amd.csp.trial_covariances``); the regularised estimators ('lwf',
    'oas', ...) are not provided and raise NotImplementedError.  ndarray in -> float64 on the GPU -> float64 ndarray
    out; CUDA tensor in (f32 / f64) -> CUDA tensor of that dtype out."""
    _param_names = ("estimator",)

    def __init__(self, estimator="scm"):
        self.estimator = estimator

    def __sklearn_tags__(self):
        return transformer_tags(required_y=False, requires_fit=False)

    def _check_params(self):
        if self.estimator != "scm":
            if isinstance(self.estimator, str) or callable(self.estimator):
                raise NotImplementedError(f"estimator={self.estimator!r}: only 'scm' is provided")
            raise ValueError(f"estimator={self.estimator!r}")

    def fit(self, X, y=None):
        self._check_params()
        return self

    def transform(self, X):
        self._check_params()
        X = check_trials(X)
        n, C_, T = X.shape
        if C_ > MAX_CHANNELS:
            raise NotImplementedError(f"{C_} channels: at most {MAX_CHANNELS} are provided")
        if C_ < 1 or T < 1:
            raise ValueError(f"X [n, C, T] needs C >= 1 and T >= 1, got {tuple(X.shape)}")
        rows = max(1, COV_CHUNK_BYTES // (C_ * max(C_, T) * 8))
        return cat_like([trial_covariances(xc) for _, xc in chunks(X, rows, "Covariances")], X, (C_, C_))

    def fit_transform(self, X, y=None, **fit_params):
        return self.fit(X, y).transform(X)


class CoSpectra(_Estimator):
    """The shape of ``pyriemann.estimation.CoSpectra``: X [n, C, T] -> the cospectral matrices [n, C, C, K], one SPD
    matrix per trial and frequency, frequency last (pyriemann's axis order) so that ``TangentSpace`` can be fitted
    per frequency on ``out[..., k]``.  It is the real part of ``connectivity.csd_array_welch`` per trial with taps
    ``np.hanning(window)``, ``n_fft = window`` and ``n_overlap = int(overlap * window)``, over the bins with
    ``fmin <= f <= fmax`` at sampling rate ``fs`` (None: 1, frequencies in cycles per sample); ``freqs_`` holds them
    after ``transform``.  **The scaling is this package's**: a density, c_k / (fs Σw²) times the mean over segments
    with each segment's mean removed; pyriemann is not installed here and parity with it is unpinned."""
    _param_names = ("window", "overlap", "fmin", "fmax", "fs")

    def __init__(self, window=128, overlap=0.75, fmin=None, fmax=None, fs=None):
        self.window, self.overlap, self.fmin, self.fmax, self.fs = window, overlap, fmin, fmax, fs

    def fit(self, X, y=None):
        return self

    def transform(self, X):
        from .connectivity import csd_array_welch
        X = check_trials(X)
        window = int(self.window)
        if not 0 <= self.overlap < 1:
            raise ValueError(f"overlap={self.overlap!r} (need 0 <= overlap < 1)")
        csd, self.freqs_ = csd_array_welch(
            X, 1.0 if self.fs is None else self.fs, 0.0 if self.fmin is None else self.fmin,
            np.inf if self.fmax is None else self.fmax, n_fft=window, n_overlap=int(self.overlap * window),
            n_per_seg=window, window=np.hanning(window), average="segments")
        re = csd.real
        return re.permute(0, 2, 3, 1).contiguous() if isinstance(re, torch.Tensor) else \
            np.ascontiguousarray(re.transpose(0, 2, 3, 1))

    def fit_transform(self, X, y=None, **fit_params):
        return self.fit(X, y).transform(X)


class TangentSpace(_Estimator):
    """Drop-in for ``pyriemann.tangentspace.TangentSpace``: ``fit`` stores ``reference_``, the Riemannian mean of the
    training covariances; ``transform`` maps X [n, C, C] to the tangent vectors [n, C (C + 1) / 2] at it.  Another
    ``metric`` and ``tsupdate=True`` are not provided and raise NotImplementedError.  Output in the input's kind."""
    _param_names = ("metric", "tsupdate")

    def __init__(self, metric="riemann", tsupdate=False):
        self.metric, self.tsupdate = metric, tsupdate

    def __sklearn_tags__(self):
        return transformer_tags(required_y=False)

    def _check_params(self):
        if self.metric != "riemann":
            raise NotImplementedError(f"metric={self.metric!r}: only 'riemann' is provided")
        if self.tsupdate:
            raise NotImplementedError("tsupdate=True is not provided")

    def fit(self, X, y=None, sample_weight=None):
        self._check_params()
        X = self._check_covs(X)
        self.reference_ = mean_riemann(X, sample_weight=sample_weight)
        return self

    def transform(self, X):
        self._fitted("reference_")
        self._check_params()
        X = self._check_covs(X)
        if X.shape[1] != self.reference_.shape[0]:
            raise ValueError(f"X has {X.shape[1]} channels, fit saw {self.reference_.shape[0]}")
        return like(tangent_space(X, self.reference_), X)

    def fit_transform(self, X, y=None, sample_weight=None):
        return self.fit(X, y, sample_weight=sample_weight).transform(X)

    def inverse_transform(self, X):
        """Tangent vectors [n, C (C + 1) / 2] -> covariances [n, C, C]: reference_^1/2 exp(S_i) reference_^1/2 (host
        work through NumPy eigh: small and rare)."""
        self._fitted("reference_")
        Cc = self.reference_.shape[0]
        T = X.detach().double().cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float64)
        if T.ndim != 2 or T.shape[1] != Cc * (Cc + 1) // 2:
            raise ValueError(f"X must be [n, {Cc * (Cc + 1) // 2}], got {T.shape}")
        iu = np.triu_indices(Cc)
        coef = np.where(iu[0] == iu[1], 1.0, np.sqrt(0.5))
        half = _host_fun(self.reference_, np.sqrt)
        out = np.empty((len(T), Cc, Cc))
        for i, t in enumerate(T):
            S = np.zeros((Cc, Cc))
            S[iu] = t * coef
            S = S + S.T - np.diag(np.diag(S))
            out[i] = half @ _host_fun(S, np.exp) @ half
        return torch.as_tensor(out).to(device=X.device, dtype=X.dtype) if isinstance(X, torch.Tensor) else out


class MDM(_Estimator):
    """Drop-in for ``pyriemann.classification.MDM`` (minimum distance to mean): ``fit`` stores the Riemannian mean
    of every class (``covmeans_`` [K, C, C], ``classes_``); ``transform`` gives the distances [n, K];
    ``predict`` the class of the nearest mean (ties to the lowest class); ``predict_proba`` softmax(−d²).  Another
    ``metric`` is not provided and raises NotImplementedError."""
    _param_names = ("metric",)

    def __init__(self, metric="riemann"):
        self.metric = metric

    def __sklearn_tags__(self):
        from sklearn.utils import ClassifierTags, InputTags, Tags, TargetTags, TransformerTags
        return Tags(estimator_type="classifier", target_tags=TargetTags(required=True),
                    transformer_tags=TransformerTags(), classifier_tags=ClassifierTags(),
                    input_tags=InputTags(three_d_array=True))

    def _check_params(self):
        if self.metric != "riemann":
            raise NotImplementedError(f"metric={self.metric!r}: only 'riemann' is provided")

    def fit(self, X, y, sample_weight=None):
        self._check_params()
        X = self._check_covs(X)
        y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
        if y.ndim != 1 or len(y) != X.shape[0]:
            raise ValueError(f"X has {X.shape[0]} matrices, y has shape {y.shape}")
        if len(y) == 0:
            raise ValueError("MDM needs at least one trial")
        self.classes_ = np.unique(y)
        self.covmeans_ = mean_riemann(X, sample_weight=sample_weight, groups=y)
        return self

    def _distances(self, X):
        self._fitted("covmeans_")
        self._check_params()
        X = self._check_covs(X)
        if X.shape[1] != self.covmeans_.shape[1]:
            raise ValueError(f"X has {X.shape[1]} channels, fit saw {self.covmeans_.shape[1]}")
        return distance_riemann(X, self.covmeans_), X

    def transform(self, X):
        d, X = self._distances(X)
        return like(d, X)

    def fit_transform(self, X, y, sample_weight=None):
        return self.fit(X, y, sample_weight=sample_weight).transform(X)

    def predict(self, X):
        d, _ = self._distances(X)
        return self.classes_[torch.argmin(d, dim=1).cpu().numpy()]      # the first minimum: ties to the lowest class

    def predict_proba(self, X):
        d, X = self._distances(X)
        return like(torch.softmax(-d.square(), dim=1), X)

    def score(self, X, y, sample_weight=None):
        y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
        return float(np.average(self.predict(X) == y, weights=sample_weight))
