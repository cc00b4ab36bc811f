"""isd_amd.csp on the host: decompose (two-class generalised eigenvectors; Pham's joint diagonaliser with
mutual-information ordering) and the argument handling of isd_amd.CSP.  No GPU.

The reference is a NumPy float64 restatement written here, independent of isd_amd/csp.py: the joint diagonaliser in
its published concatenated form (one C x KC array, explicit index vectors), its own eigh and ordering."""
import numpy as np
import pytest
import scipy.linalg

import isd_amd
from isd_amd import csp as icsp


# ------------------------------------------------------------------------------------------------- reference
def ref_pham(covs, eps=1e-6, n_iter_max=15):
    K, C, _ = covs.shape
    A = np.concatenate(list(covs), axis=1).astype(np.float64)          # C x KC
    V = np.eye(C)
    for _ in range(n_iter_max):
        decr = 0.0
        for ii in range(1, C):
            for jj in range(ii):
                Ii, Ij = np.arange(ii, K * C, C), np.arange(jj, K * C, C)
                c1, c2 = A[ii, Ii], A[jj, Ij]
                g12, g21 = np.mean(A[ii, Ij] / c1), np.mean(A[ii, Ij] / c2)
                om21, om12 = np.mean(c1 / c2), np.mean(c2 / c1)
                om = np.sqrt(om12 * om21)
                r = np.sqrt(om21 / om12)
                t1 = (r * g12 + g21) / (om + 1)
                t2 = (r * g12 - g21) / max(om - 1, 1e-9)
                h12, h21 = t1 + t2, (t1 - t2) / r
                decr += K * (g12 * h12 + g21 * h21) / 2.0
                d = 1 + np.sqrt(1 - h12 * h21)
                tau = np.array([[1, -h12 / d], [-h21 / d, 1]])
                A[[ii, jj], :] = tau @ A[[ii, jj], :]
                cols = np.stack([A[:, Ii], A[:, Ij]], axis=-1) @ tau.T  # [C, K, 2]
                A[:, Ii], A[:, Ij] = cols[..., 0], cols[..., 1]
                V[[ii, jj], :] = tau @ V[[ii, jj], :]
        if decr < C * (C - 1) * eps:
            break
    return V


def ref_decompose(covs, counts):
    covs = np.asarray(covs, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.float64)
    if len(covs) == 2:
        lam, vec = scipy.linalg.eigh(covs[0], covs[0] + covs[1])
        order = np.argsort(np.abs(lam - 0.5))[::-1]
        return vec[:, order].T, np.abs(lam - 0.5)[order]
    V = ref_pham(covs)
    p = counts / counts.sum()
    mean_cov = sum(pk * ck for pk, ck in zip(p, covs))
    out, score = [], []
    for v in V:
        v = v / np.sqrt(v @ mean_cov @ v)
        a = b = 0.0
        for pk, ck in zip(p, covs):
            q = v @ ck @ v
            a += pk * np.log(np.sqrt(q))
            b += pk * (q ** 2 - 1)
        out.append(v)
        score.append(-(a + 3.0 / 16 * b ** 2))
    order = np.argsort(score)[::-1]
    return np.array(out)[order], np.array(score)[order]


def diagonalisable(C, K):
    rng = np.random.default_rng(0)
    A = rng.standard_normal((C, C))
    d = rng.uniform(0.2, 5, size=(K, C))
    return np.array([A @ np.diag(dk) @ A.T for dk in d])


def sample_covs(C, K, seed):
    rng = np.random.default_rng(seed)
    covs = []
    for _ in range(K):
        x = rng.standard_normal((C, 4 * C)) * rng.uniform(0.5, 2.0, size=(C, 1))
        x = rng.standard_normal((C, C)) @ x / np.sqrt(C)
        covs.append(x @ x.T / x.shape[1])
    return np.array(covs)


def max_offdiag_corr(W, covs):
    worst = 0.0
    for ck in covs:
        D = W @ ck @ W.T
        s = np.sqrt(np.diag(D))
        R = np.abs(D / np.outer(s, s))
        np.fill_diagonal(R, 0.0)
        worst = max(worst, R.max())
    return worst


def align_sign(W, ref):
    return W * np.sign(np.sum(W * ref, axis=1, keepdims=True))


# ----------------------------------------------------------------------------------------------------- decompose
@pytest.mark.parametrize("C,K,bound", [(6, 3, 1e-9), (16, 5, 1e-5)])
def test_exactly_jointly_diagonalisable(C, K, bound):
    covs = diagonalisable(C, K)
    counts = np.arange(K) + 3
    W, scores = icsp.decompose(covs, counts)
    assert W.shape == (C, C) and scores.shape == (C,)
    worst = max_offdiag_corr(W, covs)
    print(f"C={C} K={K}: largest off-diagonal correlation {worst:.3g}")
    assert worst < bound
    mean_cov = np.einsum("k,kab->ab", counts / counts.sum(), covs)
    unit = np.einsum("ia,ab,ib->i", W, mean_cov, W)
    assert np.abs(unit - 1.0).max() < 1e-12
    assert np.all(np.diff(scores) <= 0)


def test_two_classes_whiten_and_diagonalise():
    covs = sample_covs(8, 2, 1)
    W, scores = icsp.decompose(covs, [5, 9])
    total = W @ (covs[0] + covs[1]) @ W.T
    assert np.abs(total - np.eye(8)).max() < 1e-10
    D = W @ covs[0] @ W.T
    lam = np.diag(D).copy()
    assert np.abs(D - np.diag(lam)).max() < 1e-10
    assert np.all(np.diff(np.abs(lam - 0.5)) <= 1e-12)             # |λ − 0.5| descending
    assert np.allclose(scores, np.abs(lam - 0.5), atol=1e-10)


@pytest.mark.parametrize("C,K", [(8, 2), (6, 3), (8, 3), (16, 5)])
def test_decompose_agrees_with_reference(C, K):
    covs = sample_covs(C, K, 10 + C + K) if K == 2 or C == 8 else diagonalisable(C, K)
    counts = np.arange(K) + 4
    W, scores = icsp.decompose(covs, counts)
    Wr, sr = ref_decompose(covs, counts)
    assert np.abs(scores - sr).max() <= 1e-10 * np.abs(sr).max()
    assert np.abs(align_sign(W, Wr) - Wr).max() <= 1e-10 * np.abs(Wr).max()


def test_decompose_rejects_bad_input():
    with pytest.raises(ValueError):
        icsp.decompose(np.eye(3)[None], [4])
    with pytest.raises(ValueError):
        icsp.decompose(np.zeros((2, 3, 4)), [1, 1])
    with pytest.raises(ValueError):
        icsp.decompose(np.stack([np.eye(3)] * 3), [1, 1])


# ------------------------------------------------------------------------------------------- argument handling
def test_exported_with_mne_signature():
    import inspect
    assert isd_amd.CSP is icsp.CSP and "CSP" in isd_amd.__all__
    params = inspect.signature(isd_amd.CSP.__init__).parameters
    assert list(params)[1:] == ["n_components", "reg", "log", "cov_est", "transform_into", "norm_trace",
                                "cov_method_params", "rank", "component_order"]
    assert [p.default for p in list(params.values())[1:]] == [4, None, None, "concat", "average_power", False, None,
                                                              None, "mutual_info"]


def test_get_set_params_round_trip():
    est = isd_amd.CSP(8, log=True, norm_trace=True)
    p = est.get_params()
    assert p["n_components"] == 8 and p["log"] is True and p["norm_trace"] is True and p["cov_est"] == "concat"
    twin = isd_amd.CSP(**p)
    assert twin.get_params() == p
    assert est.set_params(n_components=3, log=False) is est
    assert est.n_components == 3 and est.log is False
    with pytest.raises(ValueError):
        est.set_params(bogus=1)


def test_sklearn_clone():
    base = pytest.importorskip("sklearn.base")
    est = isd_amd.CSP(6, log=False, cov_est="epoch")
    est.filters_ = np.eye(4)                                        # fitted state must not be copied
    twin = base.clone(est)
    assert twin is not est and twin.get_params() == est.get_params() and not hasattr(twin, "filters_")


X8 = np.zeros((6, 8, 16))
Y8 = np.array([0, 1, 0, 1, 0, 1])


@pytest.mark.parametrize("kwargs", [dict(reg=0.1), dict(reg="ledoit_wolf"), dict(rank="full"),
                                    dict(cov_method_params={}), dict(transform_into="csp_space"),
                                    dict(component_order="alternate"), dict(n_components=17)])
def test_unprovided_options_raise_not_implemented(kwargs):
    with pytest.raises(NotImplementedError):
        isd_amd.CSP(**kwargs).fit(np.zeros((6, 32, 16)), Y8)


@pytest.mark.parametrize("X,y,kwargs", [
    (X8, np.zeros(6, dtype=int), {}),                               # fewer than two classes
    (X8[0], Y8, {}),                                                # X.ndim != 3
    (X8[..., None], Y8, {}),
    (X8, Y8[:5], {}),                                               # mismatched lengths
    (X8, Y8, dict(n_components=9)),                                 # n_components > C
    (X8, Y8, dict(cov_est="whole")),
])
def test_bad_arguments_raise_value_error(X, y, kwargs):
    with pytest.raises(ValueError):
        isd_amd.CSP(**kwargs).fit(X, y)


def test_transform_checks_state_and_channels():
    est = isd_amd.CSP(2)
    with pytest.raises(isd_amd.NotFittedError):
        est.transform(X8)
    est.filters_, est.n_channels_ = np.eye(8), 8                    # as fit leaves them
    with pytest.raises(ValueError, match="channels"):
        est.transform(np.zeros((3, 7, 16)))
    with pytest.raises(ValueError):
        est.transform(np.zeros((8, 16)))
