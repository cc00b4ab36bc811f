"""isd_amd.connectivity without a GPU: the NumPy float64 restatement that tests/test_connectivity_gpu.py holds the
kernels to (ref_csd, ref_measures) against scipy.signal.csd / coherence, the argument errors that must come before any
GPU use, the bins that faverage selects, the ABI names and the export.

CASES is shared with the GPU file: (x shape, sfreq, n_fft, n_per_seg, n_overlap, fmin, fmax)."""
import numpy as np
import pytest
import scipy.signal as ss
import torch

from test_psd_cpu import ASYM_TAPS, make_data

CASES = {
    "a": ((3, 5, 795), 250.0, 256, None, 0, 0.0, np.inf),     # C < 16, rows straddle trials, K = 129, S = 3
    "b": ((2, 4, 800), 250.0, 256, 200, 100, 1.0, 45.0),      # zero-padded segment, k_lo > 0, S = 7
    "c": ((2, 17, 300), 256.0, 128, 100, 37, 4.0, 40.0),      # one channel past a 16-tile
    "s1": ((3, 16, 256), 250.0, 256, None, 0, 9.5, 10.5),     # S = 1, one bin
    "c65": ((1, 65, 320), 128.0, 64, 64, 32, 0.0, np.inf),    # one channel past the 64-row tile
    "c128": ((2, 128, 200), 128.0, 64, 64, 48, 2.0, 40.0),    # envelope edge, bins 1..20
    "big": ((300, 4, 128), 128.0, 64, 64, 32, 0.0, np.inf),   # the over-trials split, its reduce, trial chunks
    "c1": ((2, 1, 256), 128.0, 64, 64, 0, 0.0, np.inf),       # C = 1: the CSD is the PSD
}


def ref_spectra(x, sfreq, n_fft, n_per_seg, n_overlap, fmin, fmax, window="hann", remove_dc=True):
    """x [n, C, T] float64 -> (X [n, C, S, K] complex128, freqs [K], scale [K]) under the Welch rules of psd.py."""
    T = x.shape[-1]
    nps = min(n_fft if n_per_seg is None or n_per_seg > n_fft else n_per_seg, T)
    w = ss.get_window(window, nps) if isinstance(window, str) else np.asarray(window, dtype=np.float64)
    step = nps - n_overlap
    S = (T - nps) // step + 1
    idx = np.arange(S)[:, None] * step + np.arange(nps)[None, :]
    seg = x[..., idx]                                              # [n, C, S, nps]
    if remove_dc:
        seg = seg - seg.mean(-1, keepdims=True)
    X = np.fft.rfft(seg * w, n=n_fft, axis=-1)
    f = np.fft.rfftfreq(n_fft, 1.0 / sfreq)
    keep = np.flatnonzero((f >= fmin) & (f <= fmax))
    k = np.arange(keep[0], keep[-1] + 1)
    ck = np.where((k == 0) | (2 * k == n_fft), 1.0, 2.0)
    return X[..., k], f[k], ck / (sfreq * np.sum(w * w))


def ref_csd(x, sfreq, n_fft, n_per_seg, n_overlap, fmin, fmax, window="hann", remove_dc=True, average="segments",
            unit_modulus=False):
    """-> (S, freqs, N): S[..., k, i, j] = mean X_i conj(X_j) as a density (unit_modulus: of X / |X|, unscaled);
    [n, K, C, C] for 'segments', [K, C, C] for 'trials'; N the number of (trial, segment) pairs averaged."""
    X, f, scale = ref_spectra(x, sfreq, n_fft, n_per_seg, n_overlap, fmin, fmax, window, remove_dc)
    if unit_modulus:
        m = np.abs(X)
        X = np.where(m > 0, X / np.where(m > 0, m, 1.0), 0.0)
        scale = np.ones_like(scale)
    if average == "segments":
        out = np.einsum("nisk,njsk->nkij", X, X.conj()) / X.shape[2]
        N = X.shape[2]
    else:
        out = np.einsum("nisk,njsk->kij", X, X.conj()) / (X.shape[0] * X.shape[2])
        N = X.shape[0] * X.shape[2]
    return out * scale[:, None, None], f, N


def ref_measures(S, E, N):
    """The six measures from the density S and the mean phase product E ([..., K, C, C])."""
    out = {}
    if S is not None:
        d = np.real(np.diagonal(S, axis1=-2, axis2=-1))
        cohy = S / np.sqrt(d[..., :, None] * d[..., None, :])
        out.update(cohy=cohy, coh=np.abs(cohy), imcoh=cohy.imag)
    if E is not None:
        with np.errstate(invalid="ignore", divide="ignore"):
            out.update(plv=np.abs(E), ciplv=np.abs(E.imag) / np.sqrt(1.0 - E.real ** 2),
                       ppc=(N * np.abs(E) ** 2 - 1.0) / (N - 1.0) if N > 1 else None)
    return out


@pytest.fixture(scope="module")
def con():
    from isd_amd import connectivity
    return connectivity


@pytest.mark.parametrize("window", ["hann", "taps"])
@pytest.mark.parametrize("remove_dc", [True, False])
def test_ref_csd_against_scipy(window, remove_dc):
    shape, sfreq, n_fft, nps, nov, fmin, fmax = CASES["b"]
    w = ASYM_TAPS if window == "taps" else window
    x = make_data(shape, sfreq)
    S, f, N = ref_csd(x, sfreq, n_fft, nps, nov, fmin, fmax, w, remove_dc)
    assert S.shape == (2, 45, 4, 4) and N == 7
    worst = 0.0
    for i in range(4):
        for j in range(4):                                         # scipy conjugates its first argument
            fs_, p = ss.csd(x[:, j], x[:, i], sfreq, window=w, nperseg=nps, noverlap=nov, nfft=n_fft,
                            detrend="constant" if remove_dc else False, scaling="density")
            mask = (fs_ >= fmin) & (fs_ <= fmax)
            assert np.array_equal(fs_[mask], f)
            worst = max(worst, np.abs(S[:, :, i, j] - p[:, mask]).max() / np.abs(p[:, mask]).max())
    print(f"ref_csd against scipy.signal.csd, {window}, remove_dc={remove_dc}: {worst:.2e}")
    assert worst < 1e-12
    St = ref_csd(x, sfreq, n_fft, nps, nov, fmin, fmax, w, remove_dc, average="trials")[0]
    assert np.abs(St - S.mean(0)).max() <= 1e-12 * np.abs(St).max()


def test_coh_squared_is_scipy_coherence():
    shape, sfreq, n_fft, nps, nov, fmin, fmax = CASES["b"]
    x = make_data(shape, sfreq)
    S, f, N = ref_csd(x, sfreq, n_fft, nps, nov, fmin, fmax)
    coh = ref_measures(S, None, N)["coh"]
    worst = 0.0
    for i in range(4):
        for j in range(4):
            fs_, c = ss.coherence(x[:, i], x[:, j], sfreq, window="hann", nperseg=nps, noverlap=nov, nfft=n_fft,
                                  detrend="constant")
            mask = (fs_ >= fmin) & (fs_ <= fmax)
            worst = max(worst, np.abs(coh[:, :, i, j] ** 2 - c[:, mask]).max())
    print(f"coh^2 against scipy.signal.coherence: {worst:.2e}")
    assert worst < 1e-12


def test_ref_measures_by_hand():
    rng = np.random.default_rng(0)
    u = np.exp(1j * rng.uniform(0, 2 * np.pi, (5, 3)))             # 5 pairs, 3 channels, one bin
    E = np.einsum("si,sj->ij", u, u.conj())[None] / 5
    m = ref_measures(None, E, 5)
    i, j = 2, 0
    d = np.angle(u[:, i]) - np.angle(u[:, j])
    assert abs(m["plv"][0, i, j] - abs(np.exp(1j * d).mean())) < 1e-15
    pairs = [np.cos(d[a] - d[b]) for a in range(5) for b in range(a + 1, 5)]
    assert abs(m["ppc"][0, i, j] - np.mean(pairs)) < 1e-14         # PPC is the mean cosine over distinct pairs
    e = np.exp(1j * d).mean()
    assert abs(m["ciplv"][0, i, j] - abs(e.imag) / np.sqrt(1 - e.real ** 2)) < 1e-15


def test_argument_errors_come_before_any_gpu_use(con):
    x = np.zeros((2, 4, 795))
    for name in ("pli", "dpli", "wpli", "wpli2_debiased"):
        with pytest.raises(NotImplementedError, match=name):
            con.spectral_connectivity(x, 250, method=name)
        with pytest.raises(NotImplementedError, match=name):
            con.spectral_connectivity(x, 250, method=["coh", name])
    with pytest.raises(ValueError, match="nonsense"):
        con.spectral_connectivity(x, 250, method="nonsense")
    with pytest.raises(NotImplementedError, match="multitaper"):
        con.spectral_connectivity(x, 250, mode="multitaper")
    with pytest.raises(NotImplementedError, match="wavelet"):
        con.spectral_connectivity(x, 250, mode="cwt_morlet")
    with pytest.raises(NotImplementedError, match="indices"):
        con.spectral_connectivity(x, 250, indices=([0], [1]))
    for fn in (con.csd_array_welch, con.spectral_connectivity):
        with pytest.raises(NotImplementedError, match="129 channels"):
            fn(np.zeros((1, 129, 300)), 250)
        with pytest.raises(ValueError, match=r"\[n, C, T\]"):
            fn(np.zeros(795), 250)
        with pytest.raises(ValueError, match=r"\[n, C, T\]"):
            fn(np.zeros((1, 2, 4, 795)), 250)
        with pytest.raises(TypeError, match="GPU"):
            fn(torch.zeros(2, 4, 795), 250)
        with pytest.raises(TypeError):
            fn(np.zeros((2, 4, 795), dtype=np.int32), 250)
        with pytest.raises(ValueError, match="average"):
            fn(x, 250, average="mean")
        with pytest.raises(ValueError, match="n_fft"):
            fn(np.zeros((2, 4, 200)), 250)                         # welch_design's own errors pass through
        with pytest.raises(NotImplementedError, match="n_fft"):
            fn(np.zeros((2, 4, 5000)), 250, n_fft=4096)
    with pytest.raises(ValueError, match="ppc"):
        con.spectral_connectivity(np.zeros((3, 4, 256)), 250, method="ppc", average="segments")   # S = 1
    with pytest.raises(ValueError, match="no kept frequency bin"):
        con.spectral_connectivity(x, 250, fmin=8, fmax=30, faverage=True)                          # Delta is empty


def test_faverage_bin_selection(con):
    freqs = np.arange(0.0, 51.0) * 0.5                             # 0, 0.5, ... 25 Hz
    bins = con.band_bins(freqs)                                    # BANDS_5, edges inclusive
    assert [b.tolist() for b in bins[:2]] == [list(range(1, 9)), list(range(8, 17))]
    assert bins[2].tolist() == list(range(16, 27)) and bins[3].tolist() == list(range(26, 51)) and bins[4].size == 0
    got = con.band_bins(freqs[4:], (("x", 2.0, 3.0), ("y", 100.0, 200.0)))
    assert got[0].tolist() == [0, 1, 2] and got[1].size == 0
    v = torch.arange(2 * 6 * 2 * 2, dtype=torch.float64).reshape(2, 6, 2, 2)
    m = con._band_mean(v, [np.array([0, 1]), np.array([2, 3, 4, 5])])
    assert tuple(m.shape) == (2, 2, 2, 2)
    assert torch.equal(m[:, 0], v[:, :2].mean(1)) and torch.equal(m[:, 1], v[:, 2:].mean(1))


def test_measures_in_torch_equal_the_restatement(con):
    rng = np.random.default_rng(1)
    X = rng.standard_normal((2, 3, 6, 4)) + 1j * rng.standard_normal((2, 3, 6, 4))      # [n, C, S, K]
    S = np.einsum("nisk,njsk->nkij", X, X.conj()) / 6
    U = X / np.abs(X)
    E = np.einsum("nisk,njsk->nkij", U, U.conj()) / 6
    ref = ref_measures(S, E, 6)
    off = ~np.eye(3, dtype=bool)
    for name in con.METHODS:
        got = con._measure(name, torch.as_tensor(S), torch.as_tensor(E), 6.0).numpy()
        assert got.dtype == (np.complex128 if name == "cohy" else np.float64)
        assert np.abs(got - ref[name])[..., off].max() < 1e-14, name


def test_abi_names_and_export(con):
    import isd_amd
    from isd_amd import _lib
    for name in ("isd_csd_work_bytes", "isd_csd_welch_f32", "isd_csd_welch_f64", "isd_csd_chunk_bytes"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["isd_csd_welch_f32"][1]) == 10 and len(_lib.SIGNATURES["isd_csd_work_bytes"][1]) == 6
    assert "connectivity" in isd_amd.__all__ and isd_amd.connectivity is con
    assert callable(con.csd_array_welch) and callable(con.spectral_connectivity)
    assert isd_amd.riemann.CoSpectra().get_params() == dict(window=128, overlap=0.75, fmin=None, fmax=None, fs=None)
    assert "unpinned" in con.__doc__ and "unpinned" in con.spectral_connectivity.__doc__
