"""GPU parity of the CSP transformer (csrc/csp.hip, isd_amd/csp.py) against a NumPy float64
restatement: einsum covariances, the decomposition of test_csp_cpu.py, log(mean((W X)², -1)).

Tolerances are those of test_fir_gpu.py: 1e-12 (fp64) and 1e-5 (fp32) relative to the reference's largest magnitude;
for log power, absolute in the log domain.  The end-to-end bound of 1e-8 on filters and features is an estimate: the
decomposition amplifies a covariance error by at most ~1e5 (a 1e-15 relative perturbation of the (100, 64, 250, 5)
covariances moved the first five filters by 2.4e-10), times an fp64 covariance error of ~1e-15.  Observed on an
MI355X: covariances 2.3e-15 (fp64) / 9.6e-7 (fp32), power 4.4e-16 / 7.7e-7, end to end 6.6e-16 (covs_), 6.2e-15
(filters), 2.0e-14 (features)."""
import copy

import numpy as np
import pytest
import torch

from test_csp_cpu import align_sign, ref_decompose

pytestmark = pytest.mark.gpu

TOL64, TOL32 = 1e-12, 1e-5
E2E_TOL = 1e-8
SHAPES = [(1, 1, 1), (3, 4, 7), (5, 6, 250), (4, 15, 64), (2, 64, 795), (3, 65, 129), (2, 128, 1030), (130, 9, 33)]
DTYPES = [(torch.float64, TOL64), (torch.float32, TOL32)]


@pytest.fixture(scope="module")
def isd():
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd


def _err(got, ref):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def _abs_err(got, ref):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())


def ref_cov(x):
    return np.einsum("nat,nbt->nab", x, x) / x.shape[-1]


def ref_power(x, w, log):
    p = np.mean(np.einsum("mc,nct->nmt", w, x) ** 2, axis=-1)
    return np.log(p) if log else p


def fenced(x, dtype, shift):
    """x [n, C, T] as a contiguous view into a larger NaN-filled device buffer: NaN directly before its first and
    after its last row.  shift = 1 moves the block off its 16-byte alignment."""
    pad = 64
    buf = torch.full((x.size + 2 * pad + shift,), float("nan"), dtype=dtype, device="cuda")
    view = buf[pad + shift:pad + shift + x.size].view(x.shape)
    view.copy_(torch.as_tensor(x))
    return buf, view


def data(n, C, T):
    rng = np.random.default_rng(n * 1000003 + C * 1009 + T)
    x = rng.standard_normal((n, C, T)) * rng.uniform(0.5, 2.0, size=(1, C, 1))
    if C > 1:
        x[:, 1] += 0.5 * x[:, 0]                                   # correlated channels: off-diagonals that matter
    return x


# ------------------------------------------------------------------------------------------ trial covariances
@pytest.mark.parametrize("n,C,T", SHAPES)
def test_trial_covariances(isd, n, C, T):
    x = data(n, C, T)
    ref = ref_cov(x)
    for dtype, tol in DTYPES:
        for shift in (0, 1):
            buf, xd = fenced(x, dtype, shift)
            cov = isd.csp.trial_covariances(xd)
            assert cov.shape == (n, C, C) and cov.dtype == dtype
            assert bool(torch.isfinite(cov).all()), "read a NaN sentinel"
            assert torch.equal(cov, cov.mT), "not exactly symmetric"
            err = _err(cov, ref)
            print(f"cov {dtype} shift {shift}: {err:.3g}")
            assert err < tol
        # a non-contiguous input gives the bits of its contiguous copy
        wide = torch.as_tensor(np.concatenate([x, x[..., ::-1]], axis=-1), dtype=dtype).cuda()
        assert torch.equal(isd.csp.trial_covariances(wide[..., :T]), isd.csp.trial_covariances(xd))


def test_trial_covariances_rejects_bad_input(isd):
    with pytest.raises(TypeError):
        isd.csp.trial_covariances(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError):
        isd.csp.trial_covariances(torch.zeros(2, 129, 4, device="cuda"))
    with pytest.raises(ValueError):
        isd.csp.trial_covariances(torch.zeros(3, 4, device="cuda"))
    assert isd.csp.trial_covariances(torch.zeros(0, 5, 9, device="cuda")).shape == (0, 5, 5)


# -------------------------------------------------------------------------------------------------- group mean
@pytest.mark.parametrize("C,sizes", [(6, (5, 1, 9)), (64, (3, 4)), (9, (1, 1, 40, 2))])
@pytest.mark.parametrize("norm_trace", [False, True])
def test_group_mean(isd, C, sizes, norm_trace):
    rng = np.random.default_rng(C + len(sizes))
    n = sum(sizes)
    cov = ref_cov(rng.standard_normal((n, C, 3 * C)) * rng.uniform(0.2, 3.0, size=(n, 1, 1)))
    y = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    idx = np.argsort(y, kind="stable")
    offs = np.concatenate([[0], np.cumsum(sizes)])
    for dtype, tol in DTYPES:
        covd = torch.as_tensor(cov).to("cuda", dtype)
        c = covd.double().cpu().numpy()                            # the values the kernel is given
        if norm_trace:
            c = c / np.trace(c, axis1=1, axis2=2)[:, None, None]
        ref = np.array([c[y == k].mean(0) for k in range(len(sizes))])
        out = isd.csp.cov_group_mean(covd, idx, offs, norm_trace)
        assert out.dtype == torch.float64 and out.shape == (len(sizes), C, C)
        err = _err(out, ref)
        print(f"group mean {dtype} norm_trace={norm_trace}: {err:.3g}")
        assert err < TOL64                                         # fp64 accumulation whatever the input dtype
        assert torch.equal(out, isd.csp.cov_group_mean(covd, idx, offs, norm_trace))
    with pytest.raises(ValueError):
        isd.csp.cov_group_mean(covd, idx + 1, offs, norm_trace)


# ------------------------------------------------------------------------------------------------------- power
@pytest.mark.parametrize("m", [1, 4, 8, 16])
@pytest.mark.parametrize("n,C,T", SHAPES)
def test_csp_power(isd, n, C, T, m):
    x = data(n, C, T)
    w = np.random.default_rng(m * 31 + C).standard_normal((m, C)) / np.sqrt(C)
    for dtype, tol in DTYPES:
        np_dtype = np.float64 if dtype == torch.float64 else np.float32
        for log in (True, False):
            ref = ref_power(x, w, log)
            for shift in (0, 1):
                buf, xd = fenced(x, dtype, shift)
                out = isd.csp.csp_power(xd, w.astype(np_dtype), log)
                assert out.shape == (n, m) and out.dtype == dtype
                assert bool(torch.isfinite(out).all()), "read a NaN sentinel"
                err = _abs_err(out, ref) if log else _err(out, ref)
                print(f"power {dtype} log={log} shift {shift}: {err:.3g}")
                assert err < tol
            assert torch.equal(out, isd.csp.csp_power(xd, w.astype(np_dtype), log))      # repeatable bits


def test_csp_power_rejects_bad_input(isd):
    x = torch.zeros(2, 5, 9, device="cuda")
    with pytest.raises(ValueError):
        isd.csp.csp_power(x, np.zeros((17, 5)))
    with pytest.raises(ValueError):
        isd.csp.csp_power(x, np.zeros((2, 4)))
    with pytest.raises(TypeError):
        isd.csp.csp_power(x.cpu(), np.zeros((2, 5)))


# -------------------------------------------------------------------------------------------------- end to end
def synthetic(n, C, T, K, n_test):
    """Mixing matrix A / √C from default_rng(123); class k scales the power of source k by 3 (its amplitude by √3).
    -> train and held-out sets.  The factor is read as power: with the amplitude tripled and five classes the
    mutual-information approximation itself ranks the class sources LAST (for an exact filter a = −0.258, b = 1.515,
    score = −(a + 3/16 b²) = −0.17 against 0 for a noise source), on the reference as on the estimator, and the
    pipeline then scores at chance; with the power tripled the score is +0.039 and the gap sits behind component K."""
    rng = np.random.default_rng(123)
    A = rng.standard_normal((C, C)) / np.sqrt(C)
    y = np.arange(n + n_test) % K
    s = rng.standard_normal((n + n_test, C, T))
    s[np.arange(n + n_test), y] *= np.sqrt(3.0)
    X = np.einsum("ab,nbt->nat", A, s)
    return X[:n], y[:n], X[n:], y[n:]


_cases = {}


def fitted(isd, case):
    """One fit per case for the whole module, with its NumPy reference."""
    if case not in _cases:
        n, C, T, K, m = case
        X, y, Xt, yt = synthetic(n, C, T, K, 100)
        est = isd.CSP(m, log=True).fit(X, y)
        cov = ref_cov(X)
        ref_covs = np.array([cov[y == k].mean(0) for k in range(K)])
        ref_W, ref_scores = ref_decompose(est.covs_, np.bincount(y))
        _cases[case] = dict(X=X, y=y, Xt=Xt, yt=yt, est=est, ref_covs=ref_covs, ref_W=ref_W, ref_scores=ref_scores)
    return _cases[case]


CASES = [(40, 8, 128, 2, 4), (60, 8, 256, 3, 3), (100, 64, 250, 5, 5)]


@pytest.mark.parametrize("case", CASES)
def test_end_to_end_fp64_ndarray(isd, case):
    n, C, T, K, m = case
    f = fitted(isd, case)
    est = f["est"]
    assert list(est.classes_) == list(range(K))
    assert est.covs_.shape == (K, C, C) and est.covs_.dtype == np.float64
    assert est.filters_.shape == (C, C) and est.patterns_.shape == (C, C) and est.scores_.shape == (C,)
    e_cov = _err(est.covs_, f["ref_covs"])
    W = f["ref_W"][:m]
    e_filt = _err(align_sign(est.filters_[:m], W), W)
    feats = est.transform(f["Xt"])
    assert isinstance(feats, np.ndarray) and feats.dtype == np.float64 and feats.shape == (100, m)
    e_feat = _abs_err(feats, ref_power(f["Xt"], W, True))
    print(f"case {case}: covs {e_cov:.3g}  filters {e_filt:.3g}  features {e_feat:.3g}")
    assert e_cov < TOL64
    assert e_filt < E2E_TOL
    assert e_feat < E2E_TOL
    assert np.abs(est.filters_ @ est.patterns_.T - np.eye(C)).max() < 1e-8
    power = ref_power(f["X"], W, False)
    assert _err(est.mean_, power.mean(0)) < E2E_TOL and _err(est.std_, power.std(0)) < E2E_TOL


def test_fit_in_chunks_matches_one_chunk(isd, monkeypatch):
    n, C, T, K, m = CASES[1]
    f = fitted(isd, CASES[1])
    monkeypatch.setattr(isd.csp, "COV_CHUNK_BYTES", 7 * C * T * 8)        # 7 trials per chunk, a ragged last one
    est = isd.CSP(m, log=True).fit(f["X"], f["y"])
    assert _err(est.covs_, f["est"].covs_) < TOL64
    assert _abs_err(est.transform(f["Xt"]), f["est"].transform(f["Xt"])) < E2E_TOL


def test_norm_trace_and_log_false(isd):
    n, C, T, K, m = CASES[1]
    f = fitted(isd, CASES[1])
    X, y = f["X"], f["y"]
    est = isd.CSP(m, log=False, norm_trace=True, cov_est="epoch").fit(X, y)
    cov = ref_cov(X)
    cov = cov / np.trace(cov, axis1=1, axis2=2)[:, None, None]
    assert _err(est.covs_, np.array([cov[y == k].mean(0) for k in range(K)])) < TOL64
    power = ref_power(f["Xt"], est.filters_[:m], False)
    assert _err(est.transform(f["Xt"]), (power - est.mean_) / est.std_) < E2E_TOL
    train = ref_power(X, est.filters_[:m], False)
    assert _err(est.mean_, train.mean(0)) < TOL64 * 10 and _err(est.std_, train.std(0)) < 1e-10


def test_device_path(isd):
    rng = np.random.default_rng(7)
    n, C, T, K, m = 30, 8, 300, 3, 3
    X, y, Xt, _ = synthetic(n, C, T, K, 10)
    X = X + rng.standard_normal((n, 1, T))                          # something for the band-pass to remove
    xd = torch.as_tensor(X, dtype=torch.float32).cuda()
    xf = isd.filter_data(xd, 250, 4, 40)
    est = isd.CSP(m).fit(xf, y)
    xt = isd.filter_data(torch.as_tensor(Xt, dtype=torch.float32).cuda(), 250, 4, 40)
    out = est.transform(xt)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.shape == (10, m)
    assert torch.equal(out, isd.csp.csp_power(xt, est.filters_[:m], True))
    xf64 = isd.filter_data(X, 250, 4, 40)                           # float64 ndarray
    a = isd.CSP(m).fit(xf64, y)
    b = isd.CSP(m).fit(torch.as_tensor(xf64).cuda(), torch.as_tensor(y))
    assert _err(b.covs_, a.covs_) < TOL64
    fa, fb = a.transform(xf64), b.transform(torch.as_tensor(xf64).cuda())
    assert isinstance(fa, np.ndarray) and fb.is_cuda and fb.dtype == torch.float64
    assert _abs_err(fb, fa) < TOL64
    with pytest.raises(TypeError):
        est.transform(xt.cpu())


def test_pipeline_matches_reference_features(isd):
    pytest.importorskip("sklearn")
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler
    from sklearn.svm import SVC
    case = CASES[2]
    f = fitted(isd, case)
    X, y, Xt, yt = f["X"], f["y"], f["Xt"], f["yt"]
    clf = Pipeline([("CSP", isd.CSP(8, log=True)), ("Scaler", StandardScaler()), ("SVC", SVC())])
    clf.fit(X, y)
    assert np.array_equal(clf.named_steps["CSP"].covs_, f["est"].covs_)      # the same fit, bit for bit
    W = f["ref_W"][:8]                                              # the reference run on those covariances
    ref = Pipeline([("Scaler", StandardScaler()), ("SVC", SVC())]).fit(ref_power(X, W, True), y)
    pred = clf.predict(Xt)
    assert np.array_equal(pred, ref.predict(ref_power(Xt, W, True)))
    assert clf.score(Xt, yt) == 1.0

    plain = copy.copy(f["est"]).set_params(log=False)               # mean_ / std_ are kept by every fit
    power = ref_power(Xt, plain.filters_[:5], False)
    assert _err(plain.transform(Xt), (power - plain.mean_) / plain.std_) < E2E_TOL


def test_read_only_ndarray_fits_without_a_warning(isd):
    """A read-only float64 array (np.frombuffer, a memory-mapped recording) is uploaded without torch's "not
    writable" UserWarning and gives the bits of a writeable copy: both runs execute the same code on the same values."""
    import warnings
    rng = np.random.default_rng(11)
    a = rng.standard_normal((8, 4, 64)) * np.array([1.0, 2.0, 0.5, 1.5])[None, :, None]
    y = np.array([0, 1] * 4)
    a[y == 1, 0] *= 3.0
    ro = np.frombuffer(a.tobytes()).reshape(a.shape)
    assert not ro.flags.writeable and np.array_equal(ro, a)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        est = isd.CSP(n_components=2)
        got = est.fit_transform(ro, y)
    ref_est = isd.CSP(n_components=2)
    ref = ref_est.fit_transform(a.copy(), y)
    assert got.shape == (8, 2) and np.array_equal(got, ref)
    assert np.array_equal(est.filters_, ref_est.filters_) and np.array_equal(est.covs_, ref_est.covs_)
