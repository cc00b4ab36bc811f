"""isd_amd.connectivity.spectral_connectivity_time without a GPU: the NumPy float64 restatement that
tests/test_contime_gpu.py holds the kernel to (contime_ref.ref_contime) against values worked out by hand, its symmetry
rules and bounds, the margin of the sign-based measures on the shared cases, every refusal and argument error (all of
which must come before the library is loaded or the GPU touched) and the ABI names."""
import os
import re

import numpy as np
import pytest
import torch

from contime_ref import ANTISYMMETRIC, CASES, DEAD, METHODS, make, ref_contime, sign_margin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hand_example():
    """Two channels, four samples: w_0 = 1 and w_1 = conj(s), so that s_01 = w_0 conj(w_1) = s, |s| = 5 throughout.
    Im s = 4, 3, 4, -5: sum 6, sum of moduli 16, sum of squares 66, signs + + + -; sum s = 4 + 6i."""
    s = np.array([3 + 4j, 4 + 3j, -3 + 4j, -5j])
    z = np.stack([np.ones(4, dtype=np.complex128), np.conj(s)])[None, :, None, :]      # [1, 2, 1, 4]
    want = {"coh": np.sqrt(1.0 ** 2 + 1.5 ** 2) / 5.0,             # |<s>| = |1 + 1.5i|, <|w_0|^2> = 1, <|w_1|^2> = 25
            "imcoh": 1.5 / 5.0,
            "plv": np.sqrt(0.2 ** 2 + 0.3 ** 2),                   # <u> = (4 + 6i) / 20
            "ciplv": 0.3 / np.sqrt(0.8 * 1.2),
            "pli": 2.0 / 4.0,
            "dpli": 3.0 / 4.0,
            "wpli": 6.0 / 16.0,
            "wpli2_debiased": (36.0 - 66.0) / (256.0 - 66.0)}
    return z, want


def test_restatement_on_the_hand_example():
    z, want = hand_example()
    got = ref_contime(z, METHODS, 0, 4)
    for m in METHODS:
        assert got[m].shape == (1, 1, 2, 2)
        assert abs(got[m][0, 0, 0, 1] - want[m]) <= 1e-15, (m, got[m][0, 0, 0, 1], want[m])
    # the window: the first three samples alone, Im s = 4, 3, 4: fully lagged
    got = ref_contime(z, METHODS, 0, 3)
    assert got["pli"][0, 0, 0, 1] == 1.0 and got["dpli"][0, 0, 0, 1] == 1.0
    assert abs(got["wpli"][0, 0, 0, 1] - 1.0) <= 1e-15
    assert abs(got["wpli2_debiased"][0, 0, 0, 1] - (121.0 - 41.0) / (121.0 - 41.0)) <= 1e-15
    # H(0) = 1/2: one sample with real s
    z0 = np.array([[1.0 + 0j], [2.0 + 0j]])[None, :, None, :]
    got = ref_contime(z0, ("pli", "dpli"), 0, 1)
    assert got["pli"][0, 0, 0, 1] == 0.0 and got["dpli"][0, 0, 0, 1] == 0.5


@pytest.mark.parametrize("case", ["tiles", "wide"])
def test_restatement_symmetry_and_bounds(case):
    z = make(case)
    T = z.shape[-1]
    r = ref_contime(z, METHODS, 0, T)
    C = z.shape[1]
    off = ~np.eye(C, dtype=bool)
    for m in METHODS:
        v, vt = r[m][..., off], r[m].transpose(0, 1, 3, 2)[..., off]
        assert np.isfinite(v).all(), m
        if m == "imcoh":
            assert np.array_equal(vt, -v)
        elif m == "dpli":
            assert np.abs(vt - (1.0 - v)).max() <= 1e-15
        else:
            assert m not in ANTISYMMETRIC and np.array_equal(vt, v), m
    for m in ("coh", "plv", "ciplv", "pli", "dpli", "wpli"):
        assert r[m][..., off].min() >= 0.0 and r[m][..., off].max() <= 1.0 + 1e-15, m
    assert np.abs(r["imcoh"][..., off]).max() <= 1.0 and r["wpli2_debiased"][..., off].max() <= 1.0 + 1e-15
    assert (np.abs(r["imcoh"]) <= r["coh"] + 1e-15)[..., off].all()
    assert np.abs(np.abs(2.0 * r["dpli"] - 1.0) - r["pli"])[..., off].max() <= 1e-15      # no Im s is 0 here
    assert (r["ciplv"] <= 1.0 + 1e-15)[..., off].all() and (r["plv"] >= 0)[..., off].all()
    # the diagonal of the formulas: s is real and positive there
    dg = np.einsum("nfii->nfi", r["coh"])
    assert np.abs(dg - 1.0).max() <= 1e-15
    assert np.abs(np.einsum("nfii->nfi", r["plv"]) - 1.0).max() <= 1e-15
    for m in ("imcoh", "pli"):
        assert not np.einsum("nfii->nfi", r[m]).any()
    assert (np.einsum("nfii->nfi", r["dpli"]) == 0.5).all()
    for m in ("ciplv", "wpli", "wpli2_debiased"):
        assert np.isnan(np.einsum("nfii->nfi", r[m])).all(), m


def test_restatement_lagged_and_dead():
    rng = np.random.default_rng(3)
    w = rng.standard_normal((1, 1, 2, 40)) + 1j * rng.standard_normal((1, 1, 2, 40))
    for theta in (0.3, 2.0, -1.1):
        z = np.concatenate([w, w * np.exp(-1j * theta)], axis=1)             # w_1 = w_0 e^{-i theta}
        r = ref_contime(z, METHODS, 0, 40)                                   # s_01 = |w_0|^2 e^{i theta}
        for m in ("pli", "wpli", "plv", "coh"):
            assert abs(r[m][0, :, 0, 1] - 1.0).max() <= 1e-14, (m, theta)
        assert (r["dpli"][0, :, 0, 1] == (1.0 if np.sin(theta) > 0 else 0.0)).all()
        assert abs(r["imcoh"][0, :, 0, 1] - np.sin(theta)).max() <= 1e-14
    z = make("tiles").astype(np.complex128)
    z[:, 2] = 0                                                              # a dead channel
    r = ref_contime(z, METHODS, 0, z.shape[-1])
    live = ref_contime(np.delete(z, 2, 1), METHODS, 0, z.shape[-1])
    for m in METHODS:
        row = np.delete(r[m][:, :, 2, :], 2, -1)
        want = np.full_like(row, DEAD[m])
        assert np.array_equal(row, want, equal_nan=True), m
        assert np.array_equal(np.delete(np.delete(r[m], 2, 2), 2, 3), live[m], equal_nan=True), m


def test_the_sign_margin_of_the_cases():
    """What test_contime_gpu.py asserts before it asks the sign-based measures to be exact."""
    margins = {c: sign_margin(make(c), 0, CASES[c][3]) for c in CASES}
    assert margins["one"] == np.inf
    assert all(m > 1e-6 for m in margins.values()), margins


@pytest.fixture
def no_gpu(monkeypatch):
    """Loading the library or uploading an array is a failure of the test."""
    from isd_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library / the GPU was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "to_device", boom)
    monkeypatch.setattr(torch.cuda, "is_available", boom)


def test_refusals_by_name(no_gpu):
    from isd_amd.connectivity import spectral_connectivity_time as sct
    x, f = np.zeros((2, 4, 200)), [8.0, 12.0]
    with pytest.raises(NotImplementedError, match="multitaper"):
        sct(x, f, sfreq=100, mode="multitaper")
    with pytest.raises(NotImplementedError, match="sm_times"):
        sct(x, f, sfreq=100, sm_times=0.5)
    with pytest.raises(NotImplementedError, match="sm_freqs"):
        sct(x, f, sfreq=100, sm_freqs=3)
    with pytest.raises(NotImplementedError, match="indices"):
        sct(x, f, sfreq=100, indices=(np.array([0]), np.array([1])))
    for m in ("cacoh", "mic", "mim", "gc", "gc_tr"):
        with pytest.raises(NotImplementedError, match=m):
            sct(x, f, sfreq=100, method=m)
        with pytest.raises(NotImplementedError, match=m):
            sct(x, f, sfreq=100, method=["coh", m])
    with pytest.raises(NotImplementedError, match="129"):
        sct(np.zeros((1, 129, 200)), f, sfreq=100)
    with pytest.raises(NotImplementedError, match="decim"):
        sct(x, f, sfreq=100, decim=slice(None, None, 2))


def test_argument_errors(no_gpu):
    from isd_amd.connectivity import spectral_connectivity_time as sct
    x, f = np.zeros((2, 4, 200)), [8.0, 12.0]
    with pytest.raises(TypeError):
        sct(np.zeros((2, 4, 200), dtype=np.int32), f, sfreq=100)
    with pytest.raises(TypeError):
        sct(torch.zeros(2, 4, 200), f, sfreq=100)                           # a CPU tensor
    for bad in (np.zeros(200), np.zeros((1, 2, 4, 200))):
        with pytest.raises(ValueError, match="data must be"):
            sct(bad, f, sfreq=100)
    with pytest.raises(ValueError, match="sfreq"):
        sct(x, f)
    with pytest.raises(ValueError, match="method"):
        sct(x, f, sfreq=100, method="cohy")
    with pytest.raises(ValueError, match="method"):
        sct(x, f, sfreq=100, method=[])
    with pytest.raises(ValueError, match="mode"):
        sct(x, f, sfreq=100, mode="fourier")
    with pytest.raises(ValueError, match="Nyquist"):
        sct(x, [8.0, 60.0], sfreq=100)
    with pytest.raises(ValueError, match="longer than the signal"):
        sct(x, [2.0], sfreq=100)
    with pytest.raises(ValueError, match="padding"):
        sct(x, f, sfreq=100, padding=1.0)                                   # 100 of 200 samples from each end
    with pytest.raises(ValueError, match="padding"):
        sct(x, f, sfreq=100, padding=1.0, decim=2)                          # 50 of 100 output samples from each end
    with pytest.raises(ValueError, match="padding"):
        sct(x, f, sfreq=100, padding=-0.1)
    with pytest.raises(ValueError, match="band"):
        sct(x, f, sfreq=100, faverage=True)                                 # BANDS_5 holds bands without 8 or 12 Hz
    with pytest.raises(ValueError, match="band"):
        sct(x, f, sfreq=100, faverage=True, bands=[("alpha", 8.0, 13.0), ("gamma", 30.0, 45.0)])
    with pytest.raises(ValueError, match="n=0"):
        sct(np.zeros((0, 4, 200)), f, sfreq=100, average=True)
    with pytest.raises(TypeError, match="decim"):
        sct(x, f, sfreq=100, decim=2.0)


def test_abi_names_and_header():
    from isd_amd import _lib, connectivity as con
    header = open(os.path.join(ROOT, "include", "isd_hip.h")).read()
    for name in ("isd_contime_f32", "isd_contime_f64"):
        res, args = _lib.SIGNATURES[name]
        assert res is _lib._i and len(args) == 11
        assert args[2:8] == [_lib._i64] * 6 and args[8:10] == [_lib._i, _lib._i]
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert "isd_contime_work_bytes" not in _lib.SIGNATURES and "isd_contime_work_bytes" not in header
    assert con.CONTIME_METHODS == METHODS and con.CONTIME_CHUNK_BYTES == 256 << 20
    assert con.contime_mask(["wpli", "coh"]) == 0b01000001
    assert callable(con.contime_launch)
    for m in ("pli", "dpli", "wpli", "wpli2_debiased"):                     # the Welch route still refuses them
        with pytest.raises(NotImplementedError, match=m):
            con.check_methods(m)
