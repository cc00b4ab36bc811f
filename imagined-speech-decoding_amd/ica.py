"""Independent component analysis for artifact removal: parallel FastICA with the logcosh contrast on the GPU.

``ICA`` has the constructor surface of ``mne.preprocessing.ICA`` as far as the reference uses it
(scripts/artifact_analysis.py:61: fit, then subtract blink and muscle components) and computes what MNE's default
method computes, ``sklearn.decomposition.FastICA(algorithm='parallel', whiten='unit-variance', whiten_solver='eigh',
fun='logcosh')`` fitted on the [n·T, C] matrix of concatenated trials.  It sits between ``filter_data`` and
``CSP`` / the deep models and works on the same [n, C, T] layout.

The data are never centred or whitened in memory: with μ the channel means and Kt the whitening matrix, an iteration
needs G = tanh(W Kt (x − μ)) = tanh(U x − b) with U = W Kt, b = U μ, and the sums P = Σ G xᵀ, s = Σ G, q = Σ (1 − G²),
which one pass of ``ica_step`` over the raw trials returns (csrc/ica.hip).  Everything else works on [m, C] matrices
in float64 on the host (``fastica``), as ``csp.decompose`` does.  ``get_sources`` and ``apply`` are one
``spatial_apply`` each.  There is no CPU fallback.
"""
import warnings

import numpy as np
import torch

from . import _lib
from ._estimator import Estimator, check_trials
from .csp import COV_CHUNK_BYTES, cov_group_mean, trial_covariances

MAX_COMPONENTS = 64                  # isd_ica_step_*: 1 <= m <= 64
MAX_CHANNELS = 128                   # 1 <= C <= 128
MAX_ROWS = 128                       # isd_spatial_apply_*: 1 <= R <= 128


def _like(a, x, shape, what):
    a = torch.as_tensor(a).to(device=x.device, dtype=x.dtype).contiguous()
    if tuple(a.shape) != tuple(shape):
        raise ValueError(f"{what} must be {list(shape)}, got {list(a.shape)}")
    return a


def ica_step(x, U, b, work=None):
    """x CUDA [n, C, T] (f32 / f64); U [m, C], b [m] (1 <= m <= 64; tensor or array, cast to x's dtype) ->
    (P [m, C], s [m], q [m]) as float64 CUDA tensors: with G = tanh(U x − b) per sample, P = Σ G xᵀ, s = Σ G,
    q = Σ (1 − G²) over all n·T samples.  One pass over x; bitwise repeatable.  ``work``: an optional uint8 CUDA
    scratch tensor to reuse between calls (``ica_step_work_bytes`` bytes)."""
    x = _lib.check_cuda(x, "x", MAX_CHANNELS)
    n, Cc, T = x.shape
    U = torch.as_tensor(U)
    if U.ndim != 2 or U.shape[1] != Cc or not 1 <= U.shape[0] <= MAX_COMPONENTS:
        raise ValueError(f"U must be [m, {Cc}] with 1 <= m <= {MAX_COMPONENTS}, got {tuple(U.shape)}")
    m = U.shape[0]
    U = _like(U, x, (m, Cc), "U")
    b = _like(b, x, (m,), "b")
    need = ica_step_work_bytes(n, Cc, T, m, x.dtype)
    if work is None:
        work = _lib.workspace(need, x.device)
    elif not (isinstance(work, torch.Tensor) and work.is_cuda and work.dtype == torch.uint8 and work.is_contiguous()
              and work.numel() >= need):
        raise ValueError(f"work must be a contiguous uint8 CUDA tensor of at least {need} bytes")
    P = torch.empty(m, Cc, dtype=torch.float64, device=x.device)
    s = torch.empty(m, dtype=torch.float64, device=x.device)
    q = torch.empty(m, dtype=torch.float64, device=x.device)
    fn = _lib.typed("isd_ica_step", x.dtype)
    with torch.cuda.device(x.device):
        _lib.check(fn(x.data_ptr(), U.data_ptr(), b.data_ptr(), P.data_ptr(), s.data_ptr(), q.data_ptr(),
                      work.data_ptr(), work.numel(), n, Cc, T, m, _lib.stream()))
    return P, s, q


def ica_step_work_bytes(n, C_, T, m, dtype):
    need = _lib.lib().isd_ica_step_work_bytes(n, C_, T, m, int(dtype == torch.float64))
    if need < 0:
        _lib.check(int(need))
    return int(need)


def spatial_apply(x, M, bias=None, out=None):
    """x CUDA [n, C, T] (f32 / f64); M [R, C] (1 <= R <= 128), bias [R] or None (cast to x's dtype) -> [n, R, T] of
    x's dtype: out_i = M x_i + bias[:, None].  ``out``: an optional contiguous result tensor; it must not share memory
    with x (the kernel does not work in place)."""
    x = _lib.check_cuda(x, "x", MAX_CHANNELS)
    n, Cc, T = x.shape
    M = torch.as_tensor(M)
    if M.ndim != 2 or M.shape[1] != Cc or not 1 <= M.shape[0] <= MAX_ROWS:
        raise ValueError(f"M must be [R, {Cc}] with 1 <= R <= {MAX_ROWS}, got {tuple(M.shape)}")
    R = M.shape[0]
    M = _like(M, x, (R, Cc), "M")
    bias = None if bias is None else _like(bias, x, (R,), "bias")
    if out is None:
        out = torch.empty(n, R, T, dtype=x.dtype, device=x.device)
    else:
        if not (isinstance(out, torch.Tensor) and out.device == x.device and out.dtype == x.dtype
                and tuple(out.shape) == (n, R, T) and out.is_contiguous()):
            raise ValueError(f"out must be a contiguous {x.dtype} tensor [{n}, {R}, {T}] on x's device")
        x0, o0 = x.data_ptr(), out.data_ptr()
        nbytes_x, nbytes_o = x.numel() * x.element_size(), out.numel() * out.element_size()
        if x0 < o0 + nbytes_o and o0 < x0 + nbytes_x:
            raise ValueError("out shares memory with x: spatial_apply does not work in place")
    if n:
        fn = _lib.typed("isd_spatial_apply", x.dtype)
        with torch.cuda.device(x.device):
            _lib.check(fn(x.data_ptr(), M.data_ptr(), None if bias is None else bias.data_ptr(), out.data_ptr(), n, Cc,
                          T, R, _lib.stream()))
    return out


# --------------------------------------------------------------------------------------------------- host loop
def _symdec(W):
    """Symmetric decorrelation (W Wᵀ)^-½ W."""
    from scipy.linalg import eigh
    s, u = eigh(W @ W.T)
    s = np.clip(s, np.finfo(np.float64).tiny, None)
    return np.linalg.multi_dot([u * (1.0 / np.sqrt(s)), u.T, W])


def whitening(scatter, N, m):
    """scatter [C, C] = Σ (x − μ)(x − μ)ᵀ over the N samples -> Kt [m, C] with Kt (x − μ) white (unit variance): the
    m leading eigenvectors, each divided by its root eigenvalue and signed by the first row of the eigenvector
    matrix, times √N.  Rank-deficient data raise ValueError."""
    from scipy.linalg import eigh
    scatter = np.asarray(scatter, dtype=np.float64)
    d, u = eigh(scatter)
    order = np.argsort(d)[::-1]
    d, u = d[order], u[:, order]
    if not d[m - 1] > 10 * np.finfo(np.float64).eps * d[0]:
        rank = int(np.sum(d > 10 * np.finfo(np.float64).eps * d[0]))
        raise ValueError(f"the data are rank deficient: eigenvalue {m} of the covariance is {d[m - 1]:.3g} against "
                         f"{d[0]:.3g} for the largest (rank ~{rank}); lower n_components to at most {rank}")
    d = np.sqrt(d[:m])
    u = u * np.sign(u[0])
    return np.sqrt(float(N)) * (u[:, :m] / d).T


def fastica(step, mean, scatter, N, m, w_init, tol=1e-4, max_iter=1000):
    """The FastICA fixed-point iteration on [m, C] matrices in float64.

    ``step(U, b) -> (P, s, q)`` makes the pass over the data (``ica_step`` on the GPU; any callable with float64
    arrays in the tests); ``mean`` [C] the channel means, ``scatter`` [C, C] the centred scatter matrix
    Σ x xᵀ − N μ μᵀ, ``N`` the samples per channel, ``w_init`` [m, m].  Returns (W [m, m], Kt [m, C], n_iter); the
    unmixing matrix is W Kt.  Warns with RuntimeWarning and keeps the last W if ``max_iter`` iterations do not bring
    max |abs(diag(W₁ Wᵀ)) − 1| under ``tol``."""
    mean = np.asarray(mean, dtype=np.float64).reshape(-1)
    w_init = np.asarray(w_init, dtype=np.float64)
    if w_init.shape != (m, m):
        raise ValueError(f"w_init must be [{m}, {m}], got {w_init.shape}")
    Kt = whitening(scatter, N, m)
    W = _symdec(w_init)
    Nf = float(N)
    for it in range(int(max_iter)):
        U = W @ Kt
        P, s, q = (np.asarray(v, dtype=np.float64) for v in step(U, U @ mean))
        W1 = _symdec(((P - np.outer(s, mean)) @ Kt.T) / Nf - (q / Nf)[:, None] * W)
        lim = np.max(np.abs(np.abs(np.einsum("ij,ij->i", W1, W)) - 1.0))
        W = W1
        if lim < tol:
            break
    else:
        warnings.warn(f"FastICA did not converge in {int(max_iter)} iterations (tol={tol}): consider a larger "
                      "max_iter or tol", RuntimeWarning, stacklevel=2)
    return W, Kt, it + 1


# --------------------------------------------------------------------------------------------------- estimator
class ICA(Estimator):
    """FastICA for artifact removal with the argument names of ``mne.preprocessing.ICA``: fit on [n, C, T] trials,
    ``get_sources`` for the component time courses, ``apply`` to subtract the components in ``exclude``.
    ``n_components=None`` means every channel, ``max_iter='auto'`` 1000; ``fit_params`` takes ``tol`` (1e-4),
    ``w_init`` [m, m] and ``fun_args={'alpha': 1.0}``.  Another method or contrast, a float ``n_components`` and
    alpha != 1 are not provided and raise NotImplementedError.  ndarray in -> fp64 on the GPU -> float64 ndarray out;
    CUDA tensor in (f32 / f64) -> CUDA tensor of that dtype out.  The fitted matrices are float64 ndarrays."""
    _param_names = ("n_components", "random_state", "method", "fit_params", "max_iter", "exclude")
    _fit_param_names = ("tol", "w_init", "fun_args", "fun", "algorithm")

    def __init__(self, n_components=None, *, random_state=None, method="fastica", fit_params=None, max_iter="auto",
                 exclude=()):
        self.n_components, self.random_state, self.method = n_components, random_state, method
        self.fit_params, self.max_iter, self.exclude = fit_params, max_iter, exclude

    def _check_params(self):
        """-> (tol, w_init or None, max_iter)"""
        if self.method != "fastica":
            raise NotImplementedError(f"method={self.method!r}: only 'fastica' is provided")
        m = self.n_components
        if m is not None:
            if isinstance(m, (float, np.floating)):
                raise NotImplementedError(f"n_components={m!r}: a variance fraction is not provided, give an int")
            if not isinstance(m, (int, np.integer)) or isinstance(m, bool) or m < 1:
                raise ValueError(f"n_components={m!r} (need None or a positive int)")
            if m > MAX_COMPONENTS:
                raise NotImplementedError(f"n_components={m}: at most {MAX_COMPONENTS} are provided")
        fp = dict(self.fit_params or {})
        for k in fp:
            if k not in self._fit_param_names:
                raise ValueError(f"fit_params has no {k!r} (known: {', '.join(self._fit_param_names)})")
        if fp.get("fun", "logcosh") != "logcosh":
            raise NotImplementedError(f"fun={fp['fun']!r}: only 'logcosh' is provided")
        if fp.get("algorithm", "parallel") != "parallel":
            raise NotImplementedError(f"algorithm={fp['algorithm']!r}: only 'parallel' is provided")
        fun_args = fp.get("fun_args") or {}
        if set(fun_args) - {"alpha"}:
            raise ValueError(f"fun_args={fun_args!r} (only 'alpha' is known)")
        if float(fun_args.get("alpha", 1.0)) != 1.0:
            raise NotImplementedError(f"alpha={fun_args['alpha']!r}: only alpha = 1 is provided")
        tol = float(fp.get("tol", 1e-4))
        if not tol > 0:
            raise ValueError(f"tol={tol!r} (need > 0)")
        if isinstance(self.max_iter, str):
            if self.max_iter != "auto":
                raise ValueError(f"max_iter={self.max_iter!r} (need 'auto' or a positive int)")
            max_iter = 1000
        else:
            max_iter = int(self.max_iter)
            if max_iter < 1:
                raise ValueError(f"max_iter={self.max_iter!r} (need 'auto' or a positive int)")
        return tol, fp.get("w_init"), max_iter

    @staticmethod
    def _device(X):
        """X on the GPU: a CUDA tensor as it is (contiguous), an ndarray uploaded as float64."""
        return _lib.to_device(X, isinstance(X, torch.Tensor), "ICA")

    def _exclude(self, exclude):
        ex = self.exclude if exclude is None else exclude
        ex = np.asarray(list(ex) if not np.isscalar(ex) else [ex])
        if ex.size and ex.dtype.kind not in "iu":
            raise ValueError(f"exclude={exclude!r} (need component indices)")
        ex = np.unique(ex.astype(np.int64))
        m = self.unmixing_.shape[0]
        if ex.size and (ex.min() < 0 or ex.max() >= m):
            raise ValueError(f"exclude={list(ex)} has an index outside the {m} components")
        return ex

    def fit(self, X, y=None):
        """X [n, C, T] (ndarray, or f32 / f64 CUDA tensor).  Returns self."""
        tol, w_init, max_iter = self._check_params()
        X = check_trials(X)
        n, C_, T = X.shape
        if n < 1 or T < 1:
            raise ValueError("X has no samples")
        if C_ > MAX_CHANNELS:
            raise NotImplementedError(f"{C_} channels: at most {MAX_CHANNELS} are provided")
        m = C_ if self.n_components is None else int(self.n_components)
        if m > C_:
            raise ValueError(f"n_components={m} exceeds the {C_} channels")
        if m > MAX_COMPONENTS:
            raise NotImplementedError(f"{m} components: at most {MAX_COMPONENTS} are provided")
        if w_init is None:
            w_init = np.random.RandomState(self.random_state).normal(size=(m, m))    # what sklearn draws
        w_init = np.asarray(w_init, dtype=np.float64)
        if w_init.shape != (m, m):
            raise ValueError(f"w_init must be [{m}, {m}], got {w_init.shape}")
        x = self._device(X)
        N = n * T
        mean = (x.sum(dim=(0, 2), dtype=torch.float64) / N).cpu().numpy()
        second = np.zeros((C_, C_))                                # Σ_i X_i X_iᵀ, trial chunks in order, fp64
        rows = max(1, COV_CHUNK_BYTES // (C_ * C_ * 8))
        for s0 in range(0, n, rows):
            cov = trial_covariances(x[s0:s0 + rows])
            k = cov.shape[0]
            second += cov_group_mean(cov, np.arange(k), [0, k]).cpu().numpy()[0] * (float(k) * T)
        scatter = second - N * np.outer(mean, mean)
        work = torch.empty(ica_step_work_bytes(n, C_, T, m, x.dtype), dtype=torch.uint8, device=x.device)

        def step(U, b):
            return tuple(v.cpu().numpy() for v in ica_step(x, U, b, work))

        W, Kt, n_iter = fastica(step, mean, scatter, N, m, w_init, tol, max_iter)
        self.mean_, self.whitening_ = mean, Kt
        self.unmixing_ = W @ Kt
        self.mixing_ = np.linalg.pinv(self.unmixing_)
        self.n_iter_, self.n_channels_ = n_iter, C_
        return self

    def _fitted_X(self, X, what):
        self._require_fitted("unmixing_", f"fit(X) before {what}")
        X = check_trials(X)
        if X.shape[1] != self.n_channels_:
            raise ValueError(f"X has {X.shape[1]} channels, fit saw {self.n_channels_}")
        return X

    def _spatial(self, X, M, bias):
        out = spatial_apply(self._device(X), M, bias)
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()

    def get_sources(self, X):
        """X [n, C, T] -> [n, n_components, T]: unmixing_ (X − mean_), unit variance on the data of fit."""
        X = self._fitted_X(X, "get_sources")
        return self._spatial(X, self.unmixing_, -self.unmixing_ @ self.mean_)

    def apply(self, X, exclude=None):
        """X [n, C, T] -> [n, C, T] with the components in ``exclude`` (None: ``self.exclude``) subtracted:
        X − mixing_[:, ex] unmixing_[ex] (X − mean_).  X itself is left as it is."""
        X = self._fitted_X(X, "apply")
        ex = self._exclude(exclude)
        back = self.mixing_[:, ex] @ self.unmixing_[ex]            # [C, C]
        return self._spatial(X, np.eye(self.n_channels_) - back, back @ self.mean_)
