"""GPU parity of the FastICA transformer (csrc/ica.hip, isd_amd/ica.py): the step and apply kernels against NumPy
float64, ``ICA.fit`` against ``sklearn.decomposition.FastICA`` (the oracle of test_ica_cpu.py).

Kernel tolerances are those of test_csp_gpu.py and test_fir_gpu.py: 1e-12 (fp64) and 1e-5 (fp32) relative to the
reference's largest magnitude, for each of P, s, q and for the apply output.  The fitted ``unmixing_`` must agree with
sklearn's ``components_`` to the project's end-to-end 1e-8 in fp64 (rows aligned by sign only, equal ``n_iter_``,
``mean_`` to 1e-12) and to 1e-5 for an fp32 tensor, where the oracle is fitted on the fp32-rounded data.

Observed on an MI355X (worst over the shapes and both alignments): step P 7.9e-16 / s 5.9e-16 / q 6.7e-16 in fp64 and
1.9e-7 / 4.5e-8 / 5.0e-8 in fp32; apply 6.1e-16 / 5.8e-7; ``unmixing_`` against sklearn 1.1e-13 (fp64, equal iteration
counts 9 / 9 / 7 / 14) and 3.1e-6 (fp32 tensor, the same counts); source variance within 4.2e-15 of 1."""
import numpy as np
import pytest
import torch

from test_csp_gpu import _err, fenced
from test_ica_cpu import FIT_SHAPES, SEED, align_sign, flat, make, oracle, rel_err, w_init_for

pytestmark = pytest.mark.gpu

TOL64, TOL32 = 1e-12, 1e-5
E2E_TOL = 1e-8
DTYPES = [(torch.float64, TOL64), (torch.float32, TOL32)]
STEP_SHAPES = [(1, 1, 1, 1), (3, 4, 7, 2), (2, 15, 64, 15), (2, 64, 795, 20), (3, 65, 129, 64), (2, 128, 1030, 33),
               (130, 9, 33, 9), (1, 16, 5000, 16)]                                         # n, C, T, m
APPLY_SHAPES = [(1, 1, 1, 1), (3, 4, 7, 4), (2, 64, 795, 64), (3, 65, 129, 20), (2, 128, 1030, 128), (130, 9, 33, 9)]


@pytest.fixture(scope="module")
def isd():
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd


def data(n, C, T):
    rng = np.random.default_rng(n * 1000003 + C * 1009 + T)
    x = rng.standard_normal((n, C, T)) * rng.uniform(0.5, 2.0, size=(1, C, 1)) + rng.uniform(-1, 1, size=(1, C, 1))
    if C > 1:
        x[:, 1] += 0.5 * x[:, 0]
    return x


def step_inputs(x, m):
    """Random U scaled so that U x has unit spread, random b."""
    n, C, T = x.shape
    rng = np.random.default_rng(m * 31 + C)
    U = rng.standard_normal((m, C))
    U /= max((U @ flat(x).T).std(), 1e-30)
    return U, rng.standard_normal(m)


def ref_step(x, U, b):
    X = flat(x).T
    G = np.tanh(U @ X - b[:, None])
    return G @ X.T, G.sum(1), (1.0 - G * G).sum(1)


# ---------------------------------------------------------------------------------------------------- the step
@pytest.mark.parametrize("n,C,T,m", STEP_SHAPES)
def test_ica_step(isd, n, C, T, m):
    x = data(n, C, T)
    U, b = step_inputs(x, m)
    ref = ref_step(x, U, b)
    for dtype, tol in DTYPES:
        for shift in (0, 1):
            buf, xd = fenced(x, dtype, shift)
            out = isd.ica.ica_step(xd, U, b)
            assert [tuple(o.shape) for o in out] == [(m, C), (m,), (m,)]
            assert all(o.dtype == torch.float64 and o.is_cuda for o in out)
            assert all(bool(torch.isfinite(o).all()) for o in out), "read a NaN sentinel"
            errs = [_err(o, r) for o, r in zip(out, ref)]
            print(f"step {dtype} shift {shift}: P {errs[0]:.3g}  s {errs[1]:.3g}  q {errs[2]:.3g}")
            assert max(errs) < tol
        again = isd.ica.ica_step(xd, U, b)                          # repeatable bits
        assert all(torch.equal(a, o) for a, o in zip(again, out))
        # a non-contiguous input gives the bits of its contiguous copy
        wide = torch.as_tensor(np.concatenate([x, x[..., ::-1]], axis=-1), dtype=dtype).cuda()
        view = isd.ica.ica_step(wide[..., :T], U, b)
        assert all(torch.equal(a, o) for a, o in zip(view, out))


@pytest.mark.parametrize("n,C,T,m", [(2, 64, 795, 20), (3, 4, 7, 2)])
def test_ica_step_saturated_tanh(isd, n, C, T, m):
    x = data(n, C, T)
    U, b = step_inputs(x, m)
    U = U * 100.0                                                  # |y| far beyond 50 on most samples
    ref = ref_step(x, U, b)
    for dtype, tol in DTYPES:
        buf, xd = fenced(x, dtype, 1)
        P, s, q = isd.ica.ica_step(xd, U, b)
        assert all(bool(torch.isfinite(o).all()) for o in (P, s, q))
        assert bool((s.abs() <= n * T).all()) and bool((q >= 0).all())
        err = _err(P, ref[0])
        print(f"saturated step {dtype}: P {err:.3g}")
        if dtype == torch.float64:
            assert err < tol and _err(s, ref[1]) < tol


def test_ica_step_rejects_bad_input(isd):
    x = torch.zeros(2, 5, 9, device="cuda")
    with pytest.raises(ValueError):
        isd.ica.ica_step(x, np.zeros((65, 5)), np.zeros(65))
    with pytest.raises(ValueError):
        isd.ica.ica_step(x, np.zeros((2, 4)), np.zeros(2))
    with pytest.raises(ValueError):
        isd.ica.ica_step(x, np.zeros((2, 5)), np.zeros(3))
    with pytest.raises(TypeError):
        isd.ica.ica_step(x.cpu(), np.zeros((2, 5)), np.zeros(2))
    with pytest.raises(ValueError):
        isd.ica.ica_step(x, np.zeros((2, 5)), np.zeros(2), work=torch.empty(1, dtype=torch.uint8, device="cuda"))
    from isd_amd import _lib
    assert _lib.lib().isd_ica_step_work_bytes(2, 129, 9, 2, 0) == -1
    P, s, q = isd.ica.ica_step(torch.zeros(0, 5, 9, device="cuda"), np.ones((2, 5)), np.zeros(2))
    assert float(P.abs().max()) == 0.0 and float(s.abs().max()) == 0.0 and float(q.abs().max()) == 0.0


# --------------------------------------------------------------------------------------------------- the apply
@pytest.mark.parametrize("n,C,T,R", APPLY_SHAPES)
def test_spatial_apply(isd, n, C, T, R):
    x = data(n, C, T)
    rng = np.random.default_rng(R * 31 + C)
    M, bias = rng.standard_normal((R, C)) / np.sqrt(C), rng.standard_normal(R)
    ref = np.einsum("rc,nct->nrt", M, x) + bias[None, :, None]
    for dtype, tol in DTYPES:
        for shift in (0, 1):
            xbuf, xd = fenced(x, dtype, shift)
            obuf, od = fenced(np.zeros((n, R, T)), dtype, shift)
            od.fill_(float("nan"))
            out = isd.ica.spatial_apply(xd, M, bias, out=od)
            assert out is od and bool(torch.isfinite(od).all()), "read a NaN sentinel or left an element unwritten"
            lo = 64 + shift
            assert bool(torch.isnan(obuf[:lo]).all()) and bool(torch.isnan(obuf[lo + od.numel():]).all()), \
                "wrote outside out"
            err = _err(od, ref)
            print(f"apply {dtype} shift {shift}: {err:.3g}")
            assert err < tol
        fresh = isd.ica.spatial_apply(xd, M, bias)
        assert fresh.dtype == dtype and torch.equal(fresh, od)
        assert _err(isd.ica.spatial_apply(xd, M), ref - bias[None, :, None]) < tol          # no bias


def test_spatial_apply_rejects_bad_input(isd):
    x = torch.zeros(2, 5, 9, device="cuda")
    with pytest.raises(ValueError, match="in place"):
        isd.ica.spatial_apply(x, np.eye(5), out=x)                  # out aliasing x
    flat_buf = torch.zeros(2 * 5 * 9 + 45, device="cuda")
    with pytest.raises(ValueError, match="in place"):
        isd.ica.spatial_apply(flat_buf[:90].view(2, 5, 9), np.eye(5), out=flat_buf[45:135].view(2, 5, 9))
    with pytest.raises(ValueError):
        isd.ica.spatial_apply(x, np.zeros((129, 5)))
    with pytest.raises(ValueError):
        isd.ica.spatial_apply(x, np.zeros((3, 4)))
    with pytest.raises(ValueError):
        isd.ica.spatial_apply(x, np.eye(5), out=torch.zeros(2, 5, 8, device="cuda"))
    with pytest.raises(TypeError):
        isd.ica.spatial_apply(x.cpu(), np.eye(5))
    from isd_amd import _lib
    assert _lib.lib().isd_spatial_apply_f32(x.data_ptr(), x.data_ptr(), None, x.data_ptr(), 2, 5, 9, 5, None) == -1
    assert b"same buffer" in _lib.lib().isd_last_error()
    assert isd.ica.spatial_apply(torch.zeros(0, 5, 9, device="cuda"), np.eye(5)).shape == (0, 5, 9)


# ------------------------------------------------------------------------------------------------------ the fit
_fits = {}


def fitted(isd, shape, kind):
    """One fit per (shape, kind) for the whole module."""
    if (shape, kind) not in _fits:
        n, C, T, m = shape
        x = make(n, C, T, m, SEED)[0]
        est = isd.ICA(m, fit_params=dict(w_init=w_init_for(m)))
        if kind == "ndarray":
            est.fit(x)
        elif kind == "f64":
            est.fit(torch.as_tensor(x).cuda())
        else:
            est.fit(torch.as_tensor(x, dtype=torch.float32).cuda())
        _fits[(shape, kind)] = (est, x)
    return _fits[(shape, kind)]


@pytest.mark.parametrize("kind", ["ndarray", "f64"])
@pytest.mark.parametrize("shape", FIT_SHAPES)
def test_fit_fp64_matches_sklearn(isd, shape, kind):
    n, C, T, m = shape
    est, x = fitted(isd, shape, kind)
    ref, ref_iter, ref_mean = oracle(shape, 1e-4)
    assert est.unmixing_.shape == (m, C) and est.mixing_.shape == (C, m) and est.whitening_.shape == (m, C)
    assert est.unmixing_.dtype == np.float64 and est.mean_.shape == (C,)
    err = rel_err(align_sign(est.unmixing_, ref), ref)
    e_mean = rel_err(est.mean_, ref_mean)
    print(f"fit {shape} {kind}: unmixing {err:.3g}  mean {e_mean:.3g}  n_iter {est.n_iter_} (sklearn {ref_iter})")
    assert err < E2E_TOL
    assert est.n_iter_ == ref_iter
    assert e_mean < TOL64
    assert rel_err(est.mixing_ @ est.unmixing_ @ est.mixing_, est.mixing_) < 1e-10


@pytest.mark.parametrize("shape", FIT_SHAPES)
def test_fit_fp32_matches_sklearn_on_rounded_data(isd, shape):
    """The whitening moments of fp32 input are the fp32 trial covariances of csp.hip averaged in fp64."""
    n, C, T, m = shape
    est, x = fitted(isd, shape, "f32")
    x32 = x.astype(np.float32).astype(np.float64)
    ref, ref_iter, ref_mean = oracle(shape, 1e-4, x=x32, key="fp32-rounded")
    err = rel_err(align_sign(est.unmixing_, ref), ref)
    print(f"fit {shape} f32: unmixing {err:.3g}  n_iter {est.n_iter_} (sklearn {ref_iter})")
    assert err < TOL32
    assert rel_err(est.mean_, ref_mean) < TOL32


def test_fit_default_start_and_no_convergence_warning(isd):
    shape = FIT_SHAPES[0]
    n, C, T, m = shape
    x = make(n, C, T, m, SEED)[0]
    ref, ref_iter, _ = oracle(shape, 1e-4, key="random_state", w_init=None, random_state=0)
    est = isd.ICA(random_state=0).fit(x)                           # n_components=None: every channel
    assert rel_err(align_sign(est.unmixing_, ref), ref) < E2E_TOL and est.n_iter_ == ref_iter
    with pytest.warns(RuntimeWarning, match="did not converge"):
        short = isd.ICA(m, random_state=0, max_iter=2, fit_params=dict(tol=1e-10)).fit(x)
    assert short.n_iter_ == 2 and np.isfinite(short.unmixing_).all()
    x[:, 3] = x[:, 5]
    with pytest.raises(ValueError, match="rank deficient"):
        isd.ICA(random_state=0).fit(x)


# ------------------------------------------------------------------------------------------ sources and apply
@pytest.mark.parametrize("shape", [FIT_SHAPES[0], FIT_SHAPES[1]])
def test_get_sources(isd, shape):
    n, C, T, m = shape
    est, x = fitted(isd, shape, "ndarray")
    src = est.get_sources(x)
    assert isinstance(src, np.ndarray) and src.dtype == np.float64 and src.shape == (n, m, T)
    ref = np.einsum("mc,nct->nmt", est.unmixing_, x - est.mean_[None, :, None])
    var = src.transpose(1, 0, 2).reshape(m, -1).var(axis=1)
    print(f"sources {shape}: {_err(src, ref):.3g}  max |var - 1| {np.abs(var - 1).max():.3g}")
    assert _err(src, ref) < TOL64
    assert np.abs(var - 1.0).max() < E2E_TOL
    xd = torch.as_tensor(x, dtype=torch.float32).cuda()
    s32 = est.get_sources(xd)
    assert s32.is_cuda and s32.dtype == torch.float32 and _err(s32, ref) < TOL32
    with pytest.raises(TypeError):
        est.get_sources(xd.cpu())


def test_apply(isd):
    shape = FIT_SHAPES[0]                                          # m = C = 8
    n, C, T, m = shape
    est, x = fitted(isd, shape, "ndarray")
    before = x.copy()
    same = est.apply(x, exclude=[])
    assert isinstance(same, np.ndarray) and same.shape == x.shape and _err(same, x) < TOL64
    assert _err(est.apply(x), x) < TOL64                            # exclude=None: self.exclude == ()
    none_left = est.apply(x, exclude=list(range(m)))
    assert _err(none_left, np.broadcast_to(est.mean_[None, :, None], x.shape)) < E2E_TOL
    ex = [1, 3]
    ref = x - np.einsum("ab,nbt->nat", est.mixing_[:, ex] @ est.unmixing_[ex], x - est.mean_[None, :, None])
    got = est.apply(x, exclude=ex)
    print(f"apply exclude={ex}: {_err(got, ref):.3g}")
    assert _err(got, ref) < TOL64
    assert np.array_equal(x, before)                                # X itself is left as it is
    xd = torch.as_tensor(x).cuda()
    gd = est.apply(xd, exclude=np.array(ex))
    assert gd.is_cuda and gd.dtype == torch.float64 and gd.data_ptr() != xd.data_ptr() and _err(gd, ref) < TOL64
    est6, x6 = fitted(isd, FIT_SHAPES[1], "ndarray")                # m = 6 < C = 12
    ref6 = x6 - np.einsum("ab,nbt->nat", est6.mixing_[:, [0]] @ est6.unmixing_[[0]], x6 - est6.mean_[None, :, None])
    assert _err(est6.apply(x6, exclude=[0]), ref6) < TOL64
    with pytest.raises(ValueError, match="exclude"):
        est6.apply(x6, exclude=[6])


def test_read_only_ndarray_fits_without_a_warning(isd):
    """As test_csp_gpu.py: a read-only float64 array is uploaded without torch's "not writable" UserWarning and the fit
    has the bits of the fit on a writeable copy."""
    import warnings
    a = make(8, 4, 64, 4, SEED)[0]
    ro = np.frombuffer(a.tobytes()).reshape(a.shape)
    assert not ro.flags.writeable and np.array_equal(ro, a)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                              # the fit converges too (6 iterations in sklearn)
        est = isd.ICA(4, fit_params=dict(w_init=w_init_for(4))).fit(ro)
        src = est.get_sources(ro)
    ref = isd.ICA(4, fit_params=dict(w_init=w_init_for(4))).fit(a.copy())
    assert np.array_equal(est.unmixing_, ref.unmixing_) and np.array_equal(est.mean_, ref.mean_)
    assert est.n_iter_ == ref.n_iter_ and np.array_equal(src, ref.get_sources(a.copy()))
