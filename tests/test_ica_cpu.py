"""isd_amd.ica on the host: the FastICA loop (``fastica``) driven by a NumPy float64 step, and the argument handling
of isd_amd.ICA.  No GPU.

The oracle is ``sklearn.decomposition.FastICA(algorithm='parallel', whiten='unit-variance', whiten_solver='eigh',
fun='logcosh', max_iter=1000)`` fitted on the [n·T, C] matrix of concatenated trials.  Rows are aligned by the sign of
their dot product with the oracle's row; no permutation is allowed.  The bound on ``components_`` is the project's
end-to-end 1e-8 relative to the largest entry (observed here: <= 2e-13); iteration counts and means must be equal."""
import subprocess
import sys
import warnings

import numpy as np
import pytest
from sklearn.decomposition import FastICA

import isd_amd
from isd_amd import ica as iica

E2E_TOL = 1e-8
FIT_SHAPES = [(6, 8, 250, 8), (5, 12, 129, 6), (8, 16, 257, 16), (4, 64, 795, 20)]     # n, C, T, m = sources
SEED = 7


def make(n, C, T, m_src, seed, noise=0.05):
    rng = np.random.default_rng(seed)
    S = rng.laplace(size=(n, m_src, T)); A = rng.standard_normal((C, m_src))
    x = np.einsum("cm,nmt->nct", A, S) + noise * rng.standard_normal((n, C, T))
    return x + rng.uniform(-3, 3, size=(1, C, 1)), A          # channel offsets: the mean must be handled


def w_init_for(m):
    return np.random.default_rng(1).standard_normal((m, m))


def flat(x):
    """[n, C, T] -> the [n·T, C] matrix sklearn is given."""
    return x.transpose(1, 0, 2).reshape(x.shape[1], -1).T


_oracles = {}


def oracle(shape, tol, x=None, key=None, **kwargs):
    """One sklearn fit per (shape, tol, key) for the whole session -> (components_, n_iter_, mean_)."""
    k = (shape, tol, key)
    if k not in _oracles:
        n, C, T, m = shape
        if x is None:
            x = make(n, C, T, m, SEED)[0]
        kwargs.setdefault("w_init", w_init_for(m))
        est = FastICA(n_components=m, algorithm="parallel", whiten="unit-variance", whiten_solver="eigh",
                      fun="logcosh", max_iter=1000, tol=tol, **kwargs)
        with warnings.catch_warnings():
            warnings.simplefilter("error")                         # the oracle itself must converge
            est.fit(flat(x))
        _oracles[k] = (est.components_.copy(), int(est.n_iter_), est.mean_.copy())
    return _oracles[k]


def align_sign(W, ref):
    return W * np.sign(np.sum(W * ref, axis=1, keepdims=True))


def rel_err(got, ref):
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def np_step(x):
    """The pass over the data in NumPy float64: (U, b) -> (P, s, q)."""
    X = flat(x).T                                                  # [C, N]

    def step(U, b):
        G = np.tanh(U @ X - b[:, None])
        return G @ X.T, G.sum(1), (1.0 - G * G).sum(1)
    return step


def np_moments(x):
    X = flat(x).T
    mean = X.mean(1)
    return mean, X @ X.T - X.shape[1] * np.outer(mean, mean), X.shape[1]


def np_fit(x, m, w_init, tol, max_iter=1000):
    mean, scatter, N = np_moments(x)
    W, Kt, n_iter = iica.fastica(np_step(x), mean, scatter, N, m, w_init, tol, max_iter)
    return W @ Kt, n_iter, mean


# ------------------------------------------------------------------------------------------------ the host loop
@pytest.mark.parametrize("tol", [1e-4, 1e-10])
@pytest.mark.parametrize("shape", FIT_SHAPES)
def test_fastica_matches_sklearn(shape, tol):
    n, C, T, m = shape
    x = make(n, C, T, m, SEED)[0]
    ref, ref_iter, ref_mean = oracle(shape, tol)
    unmixing, n_iter, mean = np_fit(x, m, w_init_for(m), tol)
    err = rel_err(align_sign(unmixing, ref), ref)
    print(f"{shape} tol={tol}: components {err:.3g}, n_iter {n_iter} (sklearn {ref_iter})")
    assert unmixing.shape == (m, C)
    assert err < E2E_TOL
    assert n_iter == ref_iter
    assert rel_err(mean, ref_mean) < 1e-12


def test_default_start_is_sklearns_random_state():
    shape = FIT_SHAPES[0]
    n, C, T, m = shape
    x = make(n, C, T, m, SEED)[0]
    ref, ref_iter, _ = oracle(shape, 1e-4, key="random_state", w_init=None, random_state=0)
    w0 = np.random.RandomState(0).normal(size=(m, m))
    unmixing, n_iter, _ = np_fit(x, m, w0, 1e-4)
    assert rel_err(align_sign(unmixing, ref), ref) < E2E_TOL and n_iter == ref_iter


def test_whitening_is_white_and_loop_returns_rotation():
    n, C, T, m = FIT_SHAPES[1]
    x = make(n, C, T, m, SEED)[0]
    mean, scatter, N = np_moments(x)
    Kt = iica.whitening(scatter, N, m)
    assert np.abs(Kt @ (scatter / N) @ Kt.T - np.eye(m)).max() < 1e-10
    W, Kt2, _ = iica.fastica(np_step(x), mean, scatter, N, m, w_init_for(m), 1e-4, 1000)
    assert np.array_equal(Kt, Kt2)
    assert np.abs(W @ W.T - np.eye(m)).max() < 1e-10


def test_rank_deficient_data_raise():
    n, C, T, m = FIT_SHAPES[0]
    x = make(n, C, T, m, SEED)[0]
    x[:, 3] = x[:, 5]                                              # one channel duplicated, n_components = C
    mean, scatter, N = np_moments(x)
    with pytest.raises(ValueError, match="rank deficient"):
        iica.fastica(np_step(x), mean, scatter, N, C, w_init_for(C), 1e-4, 1000)
    W, Kt, _ = iica.fastica(np_step(x), mean, scatter, N, C - 1, w_init_for(C - 1), 1e-4, 1000)    # one fewer is fine
    assert np.isfinite(W).all() and Kt.shape == (C - 1, C)


def test_no_convergence_warns_and_keeps_last_w():
    n, C, T, m = FIT_SHAPES[0]
    x = make(n, C, T, m, SEED)[0]
    mean, scatter, N = np_moments(x)
    with pytest.warns(RuntimeWarning, match="did not converge"):
        W, _, n_iter = iica.fastica(np_step(x), mean, scatter, N, m, w_init_for(m), 1e-10, 2)
    assert n_iter == 2 and np.abs(W @ W.T - np.eye(m)).max() < 1e-10
    with pytest.raises(ValueError):
        iica.fastica(np_step(x), mean, scatter, N, m, np.eye(m + 1), 1e-4, 10)


# ------------------------------------------------------------------------------------------- argument handling
def test_exported_with_mne_argument_names():
    import inspect
    assert isd_amd.ICA is iica.ICA and isd_amd.ica is iica and {"ICA", "ica"} <= set(isd_amd.__all__)
    params = inspect.signature(isd_amd.ICA.__init__).parameters
    assert list(params)[1:] == ["n_components", "random_state", "method", "fit_params", "max_iter", "exclude"]
    assert [p.default for p in list(params.values())[1:]] == [None, None, "fastica", None, "auto", ()]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in list(params.values())[2:])
    est = isd_amd.ICA(5, random_state=3)
    assert isd_amd.ICA(**est.get_params()).get_params() == est.get_params()
    assert est.set_params(n_components=4) is est and est.n_components == 4
    with pytest.raises(ValueError):
        est.set_params(bogus=1)


X8 = np.zeros((3, 8, 16))


@pytest.mark.parametrize("kwargs", [dict(method="infomax"), dict(method="picard"), dict(n_components=0.95),
                                    dict(fit_params=dict(fun="exp")), dict(fit_params=dict(fun="cube")),
                                    dict(fit_params=dict(fun_args={"alpha": 1.5})),
                                    dict(fit_params=dict(algorithm="deflation")), dict(n_components=65)])
def test_unprovided_options_raise_not_implemented(kwargs):
    with pytest.raises(NotImplementedError):
        isd_amd.ICA(**kwargs).fit(X8)


@pytest.mark.parametrize("X,kwargs", [
    (X8[0], {}),                                                    # X.ndim != 3
    (X8, dict(n_components=9)),                                     # n_components > C
    (X8, dict(n_components=0)),
    (X8, dict(max_iter=0)),
    (X8, dict(max_iter="never")),
    (X8, dict(fit_params=dict(tol=0.0))),
    (X8, dict(fit_params=dict(bogus=1))),
    (X8, dict(fit_params=dict(w_init=np.eye(3)))),                  # w_init must be [m, m]
])
def test_bad_arguments_raise_value_error(X, kwargs):
    with pytest.raises(ValueError):
        isd_amd.ICA(**kwargs).fit(X)


def test_integer_and_cpu_tensor_input_raise_type_error():
    import torch
    with pytest.raises(TypeError):
        isd_amd.ICA().fit(np.zeros((3, 8, 16), dtype=np.int64))
    with pytest.raises(TypeError):
        isd_amd.ICA().fit(torch.zeros(3, 8, 16))


def fitted_on_host(shape, exclude=()):
    """An ICA carrying what fit leaves, from the NumPy step."""
    n, C, T, m = shape
    x = make(n, C, T, m, SEED)[0]
    unmixing, n_iter, mean = np_fit(x, m, w_init_for(m), 1e-4)
    est = isd_amd.ICA(m, exclude=exclude)
    est.mean_, est.unmixing_, est.mixing_ = mean, unmixing, np.linalg.pinv(unmixing)
    est.n_iter_, est.n_channels_ = n_iter, C
    return est, x


def test_not_fitted_and_channel_checks():
    est = isd_amd.ICA(2)
    with pytest.raises(isd_amd.NotFittedError):
        est.get_sources(X8)
    with pytest.raises(isd_amd.NotFittedError):
        est.apply(X8)
    est, x = fitted_on_host(FIT_SHAPES[1])
    with pytest.raises(ValueError, match="channels"):
        est.get_sources(np.zeros((2, 11, 16)))
    with pytest.raises(ValueError):
        est.apply(np.zeros((12, 16)))


@pytest.mark.parametrize("exclude", [[6], [-1], [0, 99]])
def test_exclude_out_of_range_raises(exclude):
    est, x = fitted_on_host(FIT_SHAPES[1])                          # six components
    with pytest.raises(ValueError, match="exclude"):
        est.apply(x, exclude=exclude)
    est.exclude = exclude                                           # exclude=None means self.exclude
    with pytest.raises(ValueError, match="exclude"):
        est.apply(x)


def test_mixing_times_unmixing_is_a_projector():
    est, _ = fitted_on_host(FIT_SHAPES[1])                          # m = 6 < C = 12
    M, U = est.mixing_, est.unmixing_
    assert M.shape == (12, 6) and U.shape == (6, 12)
    assert rel_err(M @ U @ M, M) < 1e-10
    assert np.abs(U @ M - np.eye(6)).max() < 1e-10


def test_import_needs_neither_gpu_nor_library_nor_sklearn():
    code = ("import sys\n"
            "import isd_amd\n"
            "assert isd_amd.ICA().method == 'fastica'\n"
            "assert isd_amd._lib._lib is None, 'the library was loaded on import'\n"
            "assert 'sklearn' not in sys.modules and 'oracle' not in sys.modules\n"
            "import torch\n"
            "assert not torch.cuda.is_initialized()\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                       cwd=__import__("conftest").ROOT)
    assert r.returncode == 0, r.stderr
