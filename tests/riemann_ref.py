"""NumPy / SciPy float64 restatement of the Riemannian pipeline of isd_amd/riemann.py, written from the published
method (Barachant, Bonnet, Congedo & Jutten 2012; Moakher 2005 for the two-matrix mean) and independent of the
package: its own eigh-based matrix functions, the distance through the GENERALISED eigenvalues of (A, B) rather than
through a whitened matrix, explicit loops.  Shared by test_riemann_cpu.py and test_riemann_gpu.py."""
import numpy as np
import scipy.linalg


def _fun(M, f):
    lam, V = np.linalg.eigh(M)
    return (V * f(lam)) @ V.T


def sqrtm(M):
    return _fun(M, np.sqrt)


def invsqrtm(M):
    return _fun(M, lambda v: 1.0 / np.sqrt(v))


def logm(M):
    return _fun(M, np.log)


def expm(M):
    return _fun(M, np.exp)


def covariances(X):
    return np.einsum("nat,nbt->nab", X, X) / X.shape[-1]


def distance(A, B):
    """Affine-invariant distance of two SPD matrices: sqrt(sum log^2 of the generalised eigenvalues of (A, B))."""
    lam = scipy.linalg.eigvalsh(A, B)
    return float(np.sqrt(np.sum(np.log(lam) ** 2)))


def distances(covs, means):
    return np.array([[distance(c, m) for m in means] for c in covs])


def upper(S):
    """Upper triangle in np.triu_indices order, off-diagonal entries times sqrt 2."""
    iu = np.triu_indices(S.shape[-1])
    coef = np.where(iu[0] == iu[1], 1.0, np.sqrt(2.0))
    return S[..., iu[0], iu[1]] * coef


def tangent_space(covs, ref):
    W = invsqrtm(ref)
    return np.array([upper(logm(W @ c @ W.T)) for c in covs])


def mean_riemann(covs, tol=1e-8, maxiter=50, sample_weight=None):
    """-> (mean, iterations): fixed point with the adaptive step, from the weighted arithmetic mean."""
    covs = np.asarray(covs, dtype=np.float64)
    n = len(covs)
    w = np.full(n, 1.0 / n) if sample_weight is None else np.asarray(sample_weight, float) / np.sum(sample_weight)
    M = np.einsum("i,iab->ab", w, covs)
    nu, tau, crit, k = 1.0, np.finfo(np.float64).max, np.finfo(np.float64).max, 0
    while crit > tol and k < maxiter and nu > tol:
        k += 1
        M12, Mm12 = sqrtm(M), invsqrtm(M)
        J = np.zeros_like(M)
        for wi, c in zip(w, covs):
            J += wi * logm(Mm12 @ c @ Mm12)
        M = M12 @ expm(nu * J) @ M12
        crit = np.linalg.norm(J)
        h = nu * crit
        if h < tau:
            nu, tau = 0.95 * nu, h
        else:
            nu = 0.5 * nu
    return M, k


def class_means(covs, y, sample_weight=None):
    classes = np.unique(y)
    sw = None if sample_weight is None else np.asarray(sample_weight)
    out = [mean_riemann(covs[y == c], sample_weight=None if sw is None else sw[y == c]) for c in classes]
    return classes, np.array([m for m, _ in out]), np.array([k for _, k in out])


def two_matrix_mean(A, B):
    """The closed form for two matrices: A^1/2 (A^-1/2 B A^-1/2)^1/2 A^1/2."""
    A12, Am12 = sqrtm(A), invsqrtm(A)
    return A12 @ sqrtm(Am12 @ B @ Am12) @ A12


def synthetic_trials(n, C, T, seed):
    """[n, C, T] trials: white noise through a fixed random mixing with channel gains, T >= 4 C in the tests.  The
    mixing is mild (covariances of condition 30 to 100): with a unit-variance mixing the [2, 128, 1030] covariances
    reach condition 5e4, where two NumPy formulations of the distance (generalised eigenvalues, whitened log) already
    differ by 1.6e-10, more than the bound the GPU result is held to; here they agree to 4e-15."""
    rng = np.random.default_rng(seed)
    mix = 0.5 * rng.standard_normal((C, C)) / np.sqrt(C) + np.eye(C)
    gain = rng.uniform(0.5, 2.0, size=(C, 1))
    return np.einsum("ab,nbt->nat", mix, rng.standard_normal((n, C, T)) * gain)


def three_class_trials(n=90, C=8, T=250, seed=7):
    """Three classes with class-specific mixing: class k boosts sources 2k, 2k + 1 behind its own rotation.  The
    covariances stay well conditioned (about 40; their mean about 5), as band-passed EEG after whitening is."""
    rng = np.random.default_rng(seed)
    y = np.arange(n) % 3
    X = np.empty((n, C, T))
    base = 0.3 * rng.standard_normal((C, C)) / np.sqrt(C) + np.eye(C)
    mixes = []
    for k in range(3):
        g = np.ones(C)
        g[2 * k:2 * k + 2] = 3.0
        mixes.append(base @ np.diag(g) @ scipy.linalg.expm(0.3 * (lambda a: a - a.T)(rng.standard_normal((C, C)))))
    for i in range(n):
        X[i] = mixes[y[i]] @ rng.standard_normal((C, T))
    return X, y
