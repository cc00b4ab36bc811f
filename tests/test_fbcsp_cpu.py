"""isd_amd.FBCSP on the host (isd_amd/fbcsp.py, the C ABI of csrc/fb.hip's filter-bank CSP entry points): exports,
argument errors of the two entry points, the sklearn protocol, every refusal of the estimator and the band-major group
index of fit.  No GPU."""
import ctypes

import numpy as np
import pytest

import isd_amd
from isd_amd import _lib, fbcsp


# --------------------------------------------------------------------------------------------- exports and C ABI
def test_exports_and_symbols():
    import __graft_entry__
    __graft_entry__.build()
    assert isd_amd.FBCSP is fbcsp.FBCSP and "FBCSP" in isd_amd.__all__ and "fbcsp" in isd_amd.__all__
    assert callable(fbcsp.fb_trial_covariances) and callable(fbcsp.fb_csp_power)
    h = _lib.lib()
    for name in ("isd_fb_trial_cov", "isd_fb_csp_power"):
        assert name in _lib.SIGNATURES and hasattr(h, name)


def test_c_abi_argument_errors_without_gpu():
    h = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                                      # a non-null pointer that is never followed
    assert h.isd_fb_trial_cov(None, p, p, 1, 4, 8, None) == _lib.ISD_ERR_INVALID
    assert b"isd_fb_trial_cov" in h.isd_last_error() and b"null plan" in h.isd_last_error()
    assert h.isd_fb_csp_power(None, p, p, p, 1, 4, 8, 2, 1, None) == _lib.ISD_ERR_INVALID
    assert b"isd_fb_csp_power" in h.isd_last_error() and b"null plan" in h.isd_last_error()
    for C, T in ((0, 8), (129, 8), (4, 0), (4, -3)):               # the shape is refused before anything is read
        assert h.isd_fb_trial_cov(None, p, p, 1, C, T, None) == _lib.ISD_ERR_INVALID
        assert f"C={C} T={T}".encode() in h.isd_last_error()
    for C, T, m in ((0, 8, 2), (129, 8, 2), (4, 0, 2), (4, 8, 0), (4, 8, 17)):
        assert h.isd_fb_csp_power(None, p, p, p, 1, C, T, m, 1, None) == _lib.ISD_ERR_INVALID
        assert f"C={C} T={T} m={m}".encode() in h.isd_last_error()
    assert h.isd_fb_trial_cov(None, p, p, -1, 4, 8, None) == _lib.ISD_ERR_INVALID
    with pytest.raises(_lib.IsdError):
        _lib.check(h.isd_fb_csp_power(None, None, None, None, 1, 4, 8, 2, 0, None))


# ----------------------------------------------------------------------------------------------- sklearn protocol
def test_constructor_defaults_and_params_round_trip():
    import inspect
    params = inspect.signature(isd_amd.FBCSP.__init__).parameters
    assert list(params)[1:] == ["n_components", "bands", "sfreq", "order", "log", "norm_trace", "precision"]
    assert [p.default for p in list(params.values())[1:]] == [4, isd_amd.BANDS_9, 250.0, 4, None, False, "auto"]
    est = isd_amd.FBCSP(3, bands=isd_amd.BANDS_5, log=False)
    p = est.get_params()
    assert p["n_components"] == 3 and p["bands"] == isd_amd.BANDS_5 and p["log"] is False and p["sfreq"] == 250.0
    assert isd_amd.FBCSP(**p).get_params() == p
    assert est.set_params(n_components=2, precision="f64") is est
    assert est.n_components == 2 and est.precision == "f64"
    with pytest.raises(ValueError):
        est.set_params(bogus=1)
    assert callable(est.fit_transform)


def test_sklearn_clone_and_pipeline():
    base = pytest.importorskip("sklearn.base")
    from sklearn.feature_selection import SelectKBest, mutual_info_classif
    from sklearn.pipeline import Pipeline
    from sklearn.svm import SVC
    est = isd_amd.FBCSP(2, sfreq=256.0, norm_trace=True)
    est.filters_ = np.eye(4)[None]                                  # fitted state must not be copied
    twin = base.clone(est)
    assert twin is not est and twin.get_params() == est.get_params() and not hasattr(twin, "filters_")
    pipe = Pipeline([("FBCSP", isd_amd.FBCSP(2)), ("Select", SelectKBest(mutual_info_classif, k=4)), ("SVC", SVC())])
    assert base.clone(pipe).named_steps["FBCSP"].get_params() == isd_amd.FBCSP(2).get_params()


def test_not_fitted():
    est = isd_amd.FBCSP(2)
    with pytest.raises(isd_amd.NotFittedError):
        est.transform(np.zeros((3, 8, 16)))


# ------------------------------------------------------------------------------------------------------ refusals
X8 = np.zeros((6, 8, 16))
Y8 = np.array([0, 1, 0, 1, 0, 1])


def test_refusals_not_implemented():
    with pytest.raises(NotImplementedError):
        isd_amd.FBCSP(n_components=17).fit(np.zeros((6, 32, 16)), Y8)
    with pytest.raises(NotImplementedError):
        isd_amd.FBCSP(n_components=4).fit(np.zeros((6, 129, 16)), Y8)


@pytest.mark.parametrize("X,y,kwargs", [
    (X8, np.zeros(6, dtype=int), {}),                               # fewer than two classes
    (X8, Y8, dict(bands=(("low", 0.0, 4.0),))),                     # band edges outside (0, sfreq / 2)
    (X8, Y8, dict(bands=(("high", 100.0, 125.0),))),
    (X8, Y8, dict(bands=isd_amd.BANDS_5, sfreq=128.0)),             # 30 - 100 Hz at 128 Hz
    (X8, Y8, dict(bands=(("rev", 12.0, 8.0),))),
    (X8, Y8, dict(bands=())),
    (X8[0], Y8, {}),                                                # X.ndim != 3
    (X8, Y8[:5], {}),                                               # mismatched lengths
    (X8, Y8, dict(n_components=9)),                                 # n_components > C
    (X8, Y8, dict(n_components=0)),
    (X8, Y8, dict(precision="bf16")),
    (X8, Y8, dict(log="yes")),
])
def test_refusals_value_error(X, y, kwargs):
    with pytest.raises(ValueError):
        isd_amd.FBCSP(**kwargs).fit(X, y)


def test_refusals_type_error():
    import torch
    est = isd_amd.FBCSP(2)
    with pytest.raises(TypeError):
        est.fit(torch.zeros(6, 8, 16), Y8)                          # a CPU tensor: there is no CPU fallback
    with pytest.raises(TypeError):
        est.fit(np.zeros((6, 8, 16), dtype=np.int32), Y8)
    fb = object()
    with pytest.raises(TypeError):
        fbcsp.fb_trial_covariances(torch.zeros(2, 3, 4), fb)        # CPU tensor
    with pytest.raises(TypeError):
        fbcsp.fb_csp_power(torch.zeros(2, 3, 4, dtype=torch.float64), fb, np.zeros((1, 2, 3)))
    with pytest.raises(TypeError):
        fbcsp.fb_trial_covariances(np.zeros((2, 3, 4), dtype=np.float32), fb)


def test_transform_checks_channels():
    est = isd_amd.FBCSP(2)
    est.filters_, est.n_channels_, est.bands_ = np.eye(8)[None].repeat(9, 0), 8, [(4.0, 8.0)] * 9   # as fit leaves them
    with pytest.raises(ValueError, match="channels"):
        est.transform(np.zeros((3, 7, 16)))
    with pytest.raises(ValueError):
        est.transform(np.zeros((8, 16)))


# ------------------------------------------------------------------------------------------- band-major group index
@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("nb", [1, 9])
@pytest.mark.parametrize("absent", [False, True])
def test_band_major_groups_match_brute_force(K, nb, absent):
    rng = np.random.default_rng(K * 10 + nb)
    yc = rng.integers(0, K, size=23)
    if absent:
        yc[yc == K - 1] = 0                                         # a class with no trial in this chunk
    idx, offs = fbcsp.band_major_groups(yc, K, nb)
    assert idx.dtype == np.int64 and offs.dtype == np.int64 and len(offs) == nb * K + 1 and offs[0] == 0
    want = []
    for b in range(nb):
        for k in range(K):
            want.append([i * nb + b for i in range(len(yc)) if yc[i] == k])
    for g, rows in enumerate(want):
        assert list(idx[offs[g]:offs[g + 1]]) == rows, (g, rows)
    assert offs[-1] == len(idx) == nb * len(yc)
    if absent:
        assert all(offs[b * K + K] == offs[b * K + K - 1] for b in range(nb))
