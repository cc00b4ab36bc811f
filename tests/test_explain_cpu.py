"""Expected gradients without a GPU: the documented draws, the argument checks of isd_attr_mix / isd_attr_accumulate,
and a NumPy float64 restatement of the definition (the reference of the GPU tests) held against two closed forms."""
import ctypes as C

import numpy as np
import pytest


def expected_gradients_reference(f_grad, X, bg, ridx, alpha):
    """phi [n, C, T, K] float64:  phi_k[i] = (1/S) sum_s (x_i - b_r) * df_k/dx (b_r + alpha_is (x_i - b_r)),  r = ridx[i, s].

    ``f_grad(xs [m, C, T] float64) -> [m, K, C, T]``: the gradient of every logit at every row of ``xs``."""
    X, bg = np.asarray(X, np.float64), np.asarray(bg, np.float64)
    alpha = np.asarray(alpha, np.float64)
    n, S = ridx.shape
    phi = None
    for i in range(n):
        delta = X[i][None] - bg[ridx[i]]                                   # [S, C, T]
        g = np.asarray(f_grad(bg[ridx[i]] + alpha[i][:, None, None] * delta), np.float64)   # [S, K, C, T]
        if phi is None:
            phi = np.zeros((n,) + X.shape[1:] + (g.shape[1],))
        phi[i] = np.moveaxis((delta[:, None] * g).mean(0), 0, -1)
    return phi


def term_scale(f_grad, X, bg, ridx, alpha):
    """[n, K]: max_s (max|delta_s| * max|g_s|) of the reference -- the size of the terms being averaged."""
    X, bg = np.asarray(X, np.float64), np.asarray(bg, np.float64)
    out = []
    for i in range(ridx.shape[0]):
        delta = X[i][None] - bg[ridx[i]]
        g = np.asarray(f_grad(bg[ridx[i]] + np.asarray(alpha[i], np.float64)[:, None, None] * delta), np.float64)
        out.append((np.abs(delta).max(axis=(1, 2))[:, None] * np.abs(g).max(axis=(2, 3))).max(0))
    return np.stack(out)


# ---------------------------------------------------------------- draws
def test_draw_samples_is_the_two_documented_generator_calls():
    from isd_amd.explain import draw_samples
    n, S, M, seed = 6, 11, 5, 123
    ridx, alpha = draw_samples(n, S, M, seed)
    assert ridx.dtype == np.int32 and alpha.dtype == np.float32
    assert ridx.shape == (n, S) and alpha.shape == (n, S)
    assert ridx.min() >= 0 and ridx.max() < M and alpha.min() >= 0.0 and alpha.max() < 1.0
    rng = np.random.default_rng(seed)
    assert np.array_equal(ridx, rng.integers(0, M, (n, S)))
    assert np.array_equal(alpha, rng.random((n, S), dtype=np.float32))
    again = draw_samples(n, S, M, seed)
    assert np.array_equal(again[0], ridx) and np.array_equal(again[1], alpha)
    other = draw_samples(n, S, M, seed + 1)
    assert not np.array_equal(other[1], alpha)
    assert draw_samples(3, 4, 1, 0)[0].max() == 0                         # one background trial
    for bad in ((3, 0, 2), (3, 4, 0), (-1, 4, 2)):
        with pytest.raises(ValueError):
            draw_samples(*bad)


def test_package_exports_the_explainer():
    import isd_amd
    assert "explain" in isd_amd.__all__
    assert callable(isd_amd.explain.GradientExplainer) and callable(isd_amd.explain.band_heatmap)
    for est in (isd_amd.FilterbankCNNClassifier, isd_amd.FilterbankEEGNetClassifier, isd_amd.FASTHeadClassifier):
        assert callable(est.explain) and callable(est.input_gradient)


# ---------------------------------------------------------------- the C ABI without a GPU
@pytest.fixture(scope="module")
def lib():
    from isd_amd import _lib
    return _lib


def test_attr_symbols_are_declared(lib):
    assert "isd_attr_mix" in lib.SIGNATURES and "isd_attr_accumulate" in lib.SIGNATURES


def _mix(lib, ptr=1, n_pairs=1, pair0=0, S=1, E=4, M=1):
    L = lib.lib()
    p = C.c_void_p(ptr) if ptr else None
    rc = L.isd_attr_mix(p, p, p, p, p, n_pairs, pair0, S, E, M, None)
    return rc, L.isd_last_error().decode()


def _acc(lib, ptr=1, n_pairs=1, pair0=0, S=1, E=4, M=1):
    L = lib.lib()
    p = C.c_void_p(ptr) if ptr else None
    rc = L.isd_attr_accumulate(p, p, p, p, p, n_pairs, pair0, S, E, M, 1.0, None)
    return rc, L.isd_last_error().decode()


@pytest.mark.parametrize("call,name", [(_mix, "isd_attr_mix"), (_acc, "isd_attr_accumulate")])
@pytest.mark.parametrize("kw,needle", [({"ptr": 0}, "null pointer"), ({"E": 0}, "bad E"), ({"E": -4}, "bad E"),
                                       ({"S": 0}, "bad S"), ({"S": -1}, "bad S"), ({"M": 0}, "bad M"),
                                       ({"n_pairs": -1}, "bad tile"), ({"pair0": -2}, "bad tile")])
def test_attr_entry_points_reject_bad_arguments(lib, call, name, kw, needle):
    """Every check comes before the launch: the (bogus, non-null) pointers are never dereferenced."""
    rc, msg = call(lib, **kw)
    assert rc == lib.ISD_ERR_INVALID, kw
    assert name in msg and needle in msg, msg


def test_attr_null_pointer_is_checked_per_argument(lib):
    L = lib.lib()
    one = C.c_void_p(1)
    for hole in range(5):
        args = [None if k == hole else one for k in range(5)]
        assert L.isd_attr_mix(*args, 1, 0, 1, 4, 1, None) == lib.ISD_ERR_INVALID
        assert "isd_attr_mix" in L.isd_last_error().decode()
        assert L.isd_attr_accumulate(*args, 1, 0, 1, 4, 1, 1.0, None) == lib.ISD_ERR_INVALID
        assert "isd_attr_accumulate" in L.isd_last_error().decode()


def test_explainer_host_side_refusals_need_no_gpu():
    import isd_amd
    from isd_amd.explain import GradientExplainer
    bg = np.zeros((2, 3, 8), np.float32)
    with pytest.raises(isd_amd.NotFittedError):
        GradientExplainer(isd_amd.FilterbankCNNClassifier(), bg)
    with pytest.raises(isd_amd.NotFittedError):
        isd_amd.FASTHeadClassifier().explain(bg, bg)
    with pytest.raises(TypeError, match="bf16"):
        isd_amd.FilterbankCNNClassifier(precision="bf16").explain(bg, bg)
    with pytest.raises(TypeError):
        GradientExplainer(3.0, bg)
    with pytest.raises(ValueError, match="batch_size"):
        GradientExplainer(lambda x: x, bg, batch_size=0)
    with pytest.raises(ValueError, match=r"\[M, C, T\]"):
        GradientExplainer(lambda x: x, np.zeros((3, 8), np.float32))


# ---------------------------------------------------------------- the reference against closed forms
def _problem(seed, n=4, Cc=3, T=7, M=5, S=9, K=3):
    from isd_amd.explain import draw_samples
    rng = np.random.default_rng(seed)
    X, bg = rng.standard_normal((n, Cc, T)), rng.standard_normal((M, Cc, T))
    ridx, alpha = draw_samples(n, S, M, seed)
    return rng, X, bg, ridx, alpha, K


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_linear_model_closed_form_and_completeness(seed):
    rng, X, bg, ridx, alpha, K = _problem(seed)
    W = rng.standard_normal((K,) + X.shape[1:])
    phi = expected_gradients_reference(lambda xs: np.broadcast_to(W, (len(xs),) + W.shape), X, bg, ridx, alpha)
    mean_b = bg[ridx].mean(1)                                             # [n, C, T]
    want = np.moveaxis(W[None] * (X - mean_b)[:, None], 1, -1)
    assert np.abs(phi - want).max() <= 1e-12 * np.abs(want).max()
    f = lambda xs: np.einsum("kct,mct->mk", W, xs)
    total = f(X) - f(bg[ridx].reshape((-1,) + X.shape[1:])).reshape(ridx.shape + (K,)).mean(1)
    assert np.abs(phi.sum(axis=(1, 2)) - total).max() <= 1e-12 * np.abs(total).max()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_quadratic_model_closed_form(seed):
    _, X, bg, ridx, alpha, _ = _problem(seed)
    phi = expected_gradients_reference(lambda xs: xs[:, None], X, bg, ridx, alpha)      # f = |x|^2 / 2: grad = x
    delta = X[:, None] - bg[ridx]                                          # [n, S, C, T]
    want = (delta * (bg[ridx] + alpha.astype(np.float64)[:, :, None, None] * delta)).mean(1)[..., None]
    assert phi.shape == want.shape
    assert np.abs(phi - want).max() <= 1e-12 * np.abs(want).max()
