"""GPU parity of filter-bank CSP (isd_fb_trial_cov / isd_fb_csp_power in csrc/fb.hip, isd_amd/fbcsp.py).

Reference: float64 ``scipy.signal.butter(4, band, 'bandpass', fs, output='sos')`` + ``sosfilt`` on the float32-rounded
input, then einsum.  Data: the ``data(n, C, T)`` generator of test_csp_gpu.py (per-channel scales 0.5 - 2, one
correlated pair).

Bound: every test computes the same metric ``d`` for the existing two-kernel route on the same input
(``Filterbank.forward`` -> ``trial_covariances`` / ``csp_power``); the fused kernel must stay within
``max(1e-5, 4 d)``.  1e-5 is test_csp_gpu.py's fp32 bound for the product alone, 4x the margin test_tsception_gpu.py
gives a different summation order.  A case with d > 2.5e-5 fails as badly conditioned, so the bound never exceeds the
filterbank's 1e-4 gate.  Metrics: covariances max|cov - ref| / max|ref| per (trial, band), the worst over all; power
absolute in the log domain (log=True) or element-wise relative (log=False).  Every worst value is printed."""
import copy

import numpy as np
import pytest
import torch
from scipy.signal import butter, sosfilt

from test_csp_gpu import data, fenced

pytestmark = pytest.mark.gpu

FLOOR, MARGIN, ILL = 1e-5, 4.0, 2.5e-5
SHAPES = [(1, 1, 1), (3, 4, 7), (2, 15, 31), (2, 16, 32), (3, 6, 33), (5, 64, 250), (2, 64, 795), (3, 65, 129),
          (2, 128, 1030), (130, 9, 33)]
EXTRA_SHAPES = [(3, 6, 33), (5, 64, 250)]
STRUCT_SHAPES = [(3, 6, 33), (5, 64, 250), (3, 65, 129)]
MS = [1, 3, 8, 16]


@pytest.fixture(scope="module")
def isd():
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd


def plan_spec(isd, name):
    return {"b9": (isd.BANDS_9, 250.0, "auto"), "b5": (isd.BANDS_5, 250.0, "auto"), "b9_f64": (isd.BANDS_9, 250.0, "f64"),
            "b9_f32": (isd.BANDS_9, 250.0, "f32"), "one": ((("alpha", 8.0, 13.0),), 250.0, "auto")}[name]


_plans, _refs = {}, {}


def plan(isd, name):
    if name not in _plans:
        bands, fs, precision = plan_spec(isd, name)
        _plans[name] = isd.Filterbank(bands, fs, 4, precision)
    return _plans[name]


def ref_filter(x32, edges, fs, order=4):
    """float32 [n, C, T] -> float64 [n, nb, C, T]"""
    x = np.asarray(x32, dtype=np.float64)
    return np.stack([sosfilt(butter(order, [lo, hi], "bandpass", fs=fs, output="sos"), x, axis=-1) for lo, hi in edges],
                    axis=1)


def case(isd, n, C, T, name):
    """(x float32 ndarray, filtered reference [n, nb, C, T], its covariances [n, nb, C, C]); computed once."""
    key = (n, C, T, name)
    if key not in _refs:
        x = data(n, C, T).astype(np.float32)
        fb = plan(isd, name)
        y = ref_filter(x, fb.bands, fb.fs)
        y.setflags(write=False)
        cov = np.einsum("nbat,nbct->nbac", y, y) / T
        cov.setflags(write=False)
        _refs[key] = (x, y, cov)
    return _refs[key]


def cov_err(got, ref):
    got = np.asarray(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    scale = np.abs(ref).max(axis=(-2, -1), keepdims=True)
    return float((np.abs(got - ref) / np.maximum(scale, 1e-300)).max())


def pow_err(got, ref, log):
    got = np.asarray(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    return float(np.abs(got - ref).max() if log else (np.abs(got - ref) / np.abs(ref)).max())


def bound(d):
    assert d <= ILL, f"the existing route itself is at {d:.3g}: a badly conditioned case"
    return max(FLOOR, MARGIN * d)


def old_cov(isd, fb, xd):
    n, C, T = xd.shape
    return isd.csp.trial_covariances(fb.forward(xd).view(n * fb.n_bands, C, T)).view(n, fb.n_bands, C, C)


def old_power(isd, fb, xd, w, log):
    y = fb.forward(xd)
    return torch.stack([isd.csp.csp_power(y[:, b], w[b], log) for b in range(fb.n_bands)], dim=1)


def weights(nb, m, C):
    return (np.random.default_rng(m * 31 + C + nb).standard_normal((nb, m, C)) / np.sqrt(C)).astype(np.float32)


def ref_power(y, w, log):
    p = np.mean(np.einsum("bmc,nbct->nbmt", w.astype(np.float64), y) ** 2, axis=-1)
    return np.log(p) if log else p


CASES = [(s, "b9") for s in SHAPES] + [(s, p) for p in ("b5", "b9_f64", "b9_f32", "one") for s in EXTRA_SHAPES]
IDS = [f"{n}x{C}x{T}-{p}" for (n, C, T), p in CASES]


# -------------------------------------------------------------------------------------------------- covariances
@pytest.mark.parametrize("shape,name", CASES, ids=IDS)
def test_fb_trial_covariances(isd, shape, name):
    n, C, T = shape
    fb = plan(isd, name)
    if name == "b5":
        assert fb.precision == "mixed"                              # the 0.5 - 4 Hz band runs in fp64
    x, _, ref = case(isd, n, C, T, name)
    xd = torch.as_tensor(x).cuda()
    cov = isd.fbcsp.fb_trial_covariances(xd, fb)
    assert cov.shape == (n, fb.n_bands, C, C) and cov.dtype == torch.float32 and cov.is_cuda
    assert bool(torch.isfinite(cov).all())
    e, d = cov_err(cov, ref), cov_err(old_cov(isd, fb, xd), ref)
    print(f"fb cov {shape} {name}: fused {e:.3g}  existing route {d:.3g}")
    assert e <= bound(d)


# -------------------------------------------------------------------------------------------------------- power
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("shape,name", CASES, ids=IDS)
def test_fb_csp_power(isd, shape, name, m):
    n, C, T = shape
    fb = plan(isd, name)
    x, y, _ = case(isd, n, C, T, name)
    xd = torch.as_tensor(x).cuda()
    w = weights(fb.n_bands, m, C)
    for log in (True, False):
        ref = ref_power(y, w, log)
        out = isd.fbcsp.fb_csp_power(xd, fb, w, log)
        assert out.shape == (n, fb.n_bands, m) and out.dtype == torch.float32 and out.is_cuda
        assert bool(torch.isfinite(out).all())
        e, d = pow_err(out, ref, log), pow_err(old_power(isd, fb, xd, w, log), ref, log)
        print(f"fb power {shape} {name} m={m} log={log}: fused {e:.3g}  existing route {d:.3g}")
        assert e <= bound(d)
        assert torch.equal(out, isd.fbcsp.fb_csp_power(xd, fb, torch.as_tensor(w).cuda(), log))   # tensor w, same bits


def test_rejects_bad_input(isd):
    fb = plan(isd, "b9")
    x = torch.zeros(2, 5, 9, device="cuda")
    with pytest.raises(TypeError):
        isd.fbcsp.fb_trial_covariances(x.cpu(), fb)
    with pytest.raises(TypeError):
        isd.fbcsp.fb_trial_covariances(x.double(), fb)
    with pytest.raises(TypeError):
        isd.fbcsp.fb_csp_power(x.double(), fb, np.zeros((9, 2, 5)))
    with pytest.raises(ValueError):
        isd.fbcsp.fb_trial_covariances(torch.zeros(2, 129, 4, device="cuda"), fb)
    with pytest.raises(ValueError):
        isd.fbcsp.fb_trial_covariances(torch.zeros(3, 4, device="cuda"), fb)
    with pytest.raises(ValueError):
        isd.fbcsp.fb_csp_power(x, fb, np.zeros((9, 17, 5)))
    with pytest.raises(ValueError):
        isd.fbcsp.fb_csp_power(x, fb, np.zeros((8, 2, 5)))
    with pytest.raises(ValueError):
        isd.fbcsp.fb_csp_power(x, fb, np.zeros((9, 2, 4)))
    assert isd.fbcsp.fb_trial_covariances(torch.zeros(0, 5, 9, device="cuda"), fb).shape == (0, 9, 5, 5)
    assert isd.fbcsp.fb_csp_power(torch.zeros(0, 5, 9, device="cuda"), fb, np.zeros((9, 2, 5))).shape == (0, 9, 2)


# ---------------------------------------------------------------------------------------------------- structure
def both(isd, xd, fb, w):
    return isd.fbcsp.fb_trial_covariances(xd, fb), isd.fbcsp.fb_csp_power(xd, fb, w, True)


@pytest.mark.parametrize("n,C,T", STRUCT_SHAPES)
def test_symmetric_repeatable_and_batch_independent(isd, n, C, T):
    fb = plan(isd, "b9")
    x = case(isd, n, C, T, "b9")[0]
    xd = torch.as_tensor(x).cuda()
    w = weights(fb.n_bands, 3, C)
    cov, pw = both(isd, xd, fb, w)
    assert torch.equal(cov, cov.mT), "not exactly symmetric"
    cov2, pw2 = both(isd, xd, fb, w)
    assert torch.equal(cov, cov2) and torch.equal(pw, pw2), "two calls differ"
    for i in (0, n - 1):                                            # a trial alone = the trial inside the batch
        ci, pi = both(isd, xd[i:i + 1].clone(), fb, w)
        assert torch.equal(ci[0], cov[i]) and torch.equal(pi[0], pw[i]), f"trial {i} depends on the batch"
    wide = torch.as_tensor(np.concatenate([x, x[..., ::-1]], axis=-1)).cuda()
    cn, pn = both(isd, wide[..., :T], fb, w)                        # non-contiguous input
    assert torch.equal(cn, cov) and torch.equal(pn, pw)


@pytest.mark.parametrize("n,C,T", STRUCT_SHAPES)
def test_nan_fences_and_neighbours(isd, n, C, T):
    fb = plan(isd, "b9")
    x = case(isd, n, C, T, "b9")[0]
    w = weights(fb.n_bands, 3, C)
    cov, pw = both(isd, torch.as_tensor(x).cuda(), fb, w)
    for shift in (0, 1):                                            # shift 1: off 16-byte alignment
        buf, xd = fenced(x, torch.float32, shift)
        cf, pf = both(isd, xd, fb, w)
        assert bool(torch.isfinite(cf).all()) and bool(torch.isfinite(pf).all()), "read a NaN sentinel"
        assert torch.equal(cf, cov) and torch.equal(pf, pw)
    # NaN in the samples of the buffer's next trial does not reach the last trial
    more = torch.full((n + 1, C, T), float("nan"), device="cuda")
    more[:n] = torch.as_tensor(x)
    cm, pm = both(isd, more[:n], fb, w)
    assert torch.equal(cm, cov) and torch.equal(pm, pw)
    # ... and a NaN trial inside the batch stays in its own results
    if n >= 3:
        more[1] = float("nan")
        cm, pm = both(isd, more[:n], fb, w)
        assert torch.equal(cm[0], cov[0]) and torch.equal(cm[2], cov[2])
        assert torch.equal(pm[0], pw[0]) and torch.equal(pm[2], pw[2])


@pytest.mark.parametrize("n,C,T", STRUCT_SHAPES)
@pytest.mark.parametrize("name", ["b9", "b5"])
def test_band_order_is_the_callers(isd, n, C, T, name):
    bands, fs, precision = plan_spec(isd, name)
    fb = plan(isd, name)
    x = case(isd, n, C, T, "b9")[0]
    xd = torch.as_tensor(x).cuda()
    w = weights(fb.n_bands, 3, C)
    cov, pw = both(isd, xd, fb, w)
    perm = np.random.default_rng(len(bands)).permutation(len(bands))
    fbp = isd.Filterbank([bands[p] for p in perm], fs, 4, precision)
    cp, pp = both(isd, xd, fbp, w[perm])
    idx = torch.as_tensor(perm).cuda()
    assert torch.equal(cp, cov[:, idx]) and torch.equal(pp, pw[:, idx])


# ---------------------------------------------------------------------------------------------------- estimator
EST_CASES = [(90, 8, 250, 3, 2, "b9"), (60, 6, 200, 2, 2, "b5"), (100, 64, 250, 5, 4, "b9")]
FREQS = [6.0, 18.0, 30.0, 10.0, 26.0]
FS = 250.0


def synthetic(n, C, T, K, seed):
    """Class k carries a 1.5-amplitude sinusoid at FREQS[k] Hz (random phase) through a fixed random spatial pattern,
    plus unit white noise."""
    A = np.random.default_rng(123).standard_normal((C, len(FREQS)))
    rng = np.random.default_rng(seed)
    y = np.arange(n) % K
    t = np.arange(T) / FS
    s = 1.5 * np.sin(2 * np.pi * np.asarray(FREQS)[y][:, None] * t[None, :] + rng.uniform(0, 2 * np.pi, (n, 1)))
    X = A[:, y].T[:, :, None] * s[:, None, :] + rng.standard_normal((n, C, T))
    return X, y


_fits = {}


def fitted(isd, c):
    if c not in _fits:
        n, C, T, K, m, name = c
        bands = plan_spec(isd, name)[0]
        X, y = synthetic(n, C, T, K, 1)
        est = isd.FBCSP(m, bands=bands, sfreq=FS).fit(X, y)
        _fits[c] = dict(X=X, y=y, est=est, bands=bands)
    return _fits[c]


@pytest.mark.parametrize("c", EST_CASES, ids=[f"C{c[1]}-K{c[3]}-{c[5]}" for c in EST_CASES])
def test_estimator(isd, c):
    n, C, T, K, m, name = c
    f = fitted(isd, c)
    est, X, y = f["est"], f["X"], f["y"]
    nb = len(f["bands"])
    fb = plan(isd, name)
    assert est.bands_ == fb.bands and list(est.classes_) == list(range(K)) and est.n_channels_ == C
    assert est.covs_.shape == (nb, K, C, C) and est.covs_.dtype == np.float64
    assert est.filters_.shape == (nb, C, C) and est.scores_.shape == (nb, C) and est.patterns_.shape == (nb, C, C)
    assert est.mean_.shape == (nb * m,) and est.std_.shape == (nb * m,)
    x32 = X.astype(np.float32)
    xd = torch.as_tensor(x32).cuda()
    yf = ref_filter(x32, fb.bands, FS)
    cov = np.einsum("nbat,nbct->nbac", yf, yf) / T
    ref_covs = np.stack([cov[y == k].mean(0) for k in range(K)], axis=1)            # [nb, K, C, C]
    oc = old_cov(isd, fb, xd).double().cpu().numpy()
    old_covs = np.stack([oc[y == k].mean(0) for k in range(K)], axis=1)
    e, d = cov_err(est.covs_, ref_covs), cov_err(old_covs, ref_covs)
    print(f"estimator {c}: covs_ fused {e:.3g}  existing route {d:.3g}")
    assert e <= bound(d)
    counts = np.bincount(y)
    for b in range(nb):
        W, s = isd.csp.decompose(est.covs_[b], counts)
        assert np.abs(est.filters_[b] - W).max() <= 1e-12 * np.abs(W).max()
        assert np.abs(est.scores_[b] - s).max() <= 1e-12 * max(np.abs(s).max(), 1e-300)
        assert np.abs(est.filters_[b] @ est.patterns_[b].T - np.eye(C)).max() < 1e-6
    # transform against the fp64 reference evaluated with the estimator's own filters
    Xt, _ = synthetic(40, C, T, K, 2)
    xt32 = Xt.astype(np.float32)
    xtd = torch.as_tensor(xt32).cuda()
    w = est.filters_[:, :m].astype(np.float32)
    ref = ref_power(ref_filter(xt32, fb.bands, FS), w, True).reshape(40, nb * m)
    out = est.transform(Xt)
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == (40, nb * m)
    e = pow_err(out, ref, True)
    d = pow_err(old_power(isd, fb, xtd, w, True).reshape(40, nb * m), ref, True)
    print(f"estimator {c}: transform fused {e:.3g}  existing route {d:.3g}")
    assert e <= bound(d)
    out_t = est.transform(xtd)
    assert isinstance(out_t, torch.Tensor) and out_t.is_cuda and out_t.dtype == torch.float32
    assert np.array_equal(out_t.double().cpu().numpy(), out)        # the same values either way
    with pytest.raises(TypeError):
        est.transform(xtd.double())
    with pytest.raises(TypeError):
        est.transform(xtd.cpu())
    # log=False: the z-scored power
    plain = copy.copy(est).set_params(log=False)
    power = isd.fbcsp.fb_csp_power(xtd, fb, w, False).double().cpu().numpy().reshape(40, nb * m)
    assert np.abs(plain.transform(Xt) - (power - est.mean_) / est.std_).max() < 1e-12
    train = isd.fbcsp.fb_csp_power(xd, fb, w, False).double().cpu().numpy().reshape(n, nb * m)
    assert np.abs(est.mean_ - train.mean(0)).max() <= 1e-12 * np.abs(train).max()
    assert np.abs(est.std_ - train.std(0)).max() <= 1e-12 * np.abs(train).max()


@pytest.mark.parametrize("c", EST_CASES[:2], ids=["K3-b9", "K2-b5"])
def test_fit_in_chunks_matches_one_chunk(isd, monkeypatch, c):
    n, C, T, K, m, name = c
    f = fitted(isd, c)
    nb = len(f["bands"])
    monkeypatch.setattr(isd.fbcsp, "COV_CHUNK_BYTES", 7 * nb * C * max(C, T) * 4)   # 7 trials per chunk, a ragged last
    est = isd.FBCSP(m, bands=f["bands"], sfreq=FS).fit(f["X"], f["y"])
    ref = f["est"].covs_
    assert np.abs(est.covs_ - ref).max() <= 1e-12 * np.abs(ref).max()
    xd = torch.as_tensor(f["X"], dtype=torch.float32).cuda()        # a tensor fit is the same fit
    est_t = isd.FBCSP(m, bands=f["bands"], sfreq=FS).fit(xd, torch.as_tensor(f["y"]))
    assert np.abs(est_t.covs_ - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("c", EST_CASES[:2], ids=["K3-b9", "K2-b5"])
def test_held_out_accuracy(isd, c):
    n, C, T, K, m, name = c
    f = fitted(isd, c)
    est = f["est"]
    F = est.transform(f["X"])
    mu, sd = F.mean(0), F.std(0)
    cent = np.stack([((F - mu) / sd)[f["y"] == k].mean(0) for k in range(K)])
    Xt, yt = synthetic(200, C, T, K, 7)
    Ft = (est.transform(Xt) - mu) / sd
    pred = np.argmin(((Ft[:, None, :] - cent[None]) ** 2).sum(-1), axis=1)
    acc = float((pred == yt).mean())
    print(f"held-out accuracy {c}: {acc:.3f}")
    assert acc >= 0.9


def test_pipeline(isd):
    pytest.importorskip("sklearn")
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler
    from sklearn.svm import SVC
    c = EST_CASES[0]
    n, C, T, K, m, name = c
    f = fitted(isd, c)
    clf = Pipeline([("FBCSP", isd.FBCSP(m, bands=f["bands"], sfreq=FS)), ("Scaler", StandardScaler()), ("SVC", SVC())])
    clf.fit(f["X"], f["y"])
    assert np.array_equal(clf.named_steps["FBCSP"].covs_, f["est"].covs_)       # the same fit, bit for bit
    Xt, yt = synthetic(60, C, T, K, 9)
    pred = clf.predict(Xt)
    assert pred.shape == (60,) and set(pred) <= set(range(K))
    print(f"pipeline accuracy: {float((pred == yt).mean()):.3f}")
