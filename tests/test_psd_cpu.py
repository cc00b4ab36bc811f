"""isd_amd.psd without a GPU: welch_design (segment rules, window, bins, scale) restated in NumPy float64 against
scipy.signal.welch, the median bias against scipy's, band_power against a hand sum, and the argument errors.

PARAMS is shared with tests/test_psd_gpu.py: (x shape, sfreq, n_fft, n_per_seg, n_overlap, fmin, fmax)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.signal as ss

PARAMS = {
    "a": ((3, 5, 795), 250.0, 256, None, 0, 0.0, np.inf),     # the reference's trial; S = 3; K = 129; 27 unused samples
    "b": ((2, 4, 800), 250.0, 256, 200, 100, 1.0, 45.0),      # zero-padded segment, overlap, S = 7, K = 45
    "c": ((2, 3, 300), 256.0, 128, 100, 37, 4.0, 40.0),       # step coprime to everything, K = 19
    "d": ((2, 2, 257), 250.0, 255, None, 0, 0.0, np.inf),     # odd n_fft (no Nyquist bin), S = 1
    # one row, one segment, one bin (k = 10 at 9.766 Hz).  The bins lie 0.977 Hz apart, so the band 10 .. 10.5 Hz holds
    # none and is an error (test_argument_errors); the one-bin case takes the band half a hertz lower.
    "e": ((1, 1, 256), 250.0, 256, None, 0, 9.5, 10.5),
    "f17": ((17, 1, 64), 128.0, 64, 64, 32, 0.0, np.inf),     # one row past a 16-row tile
    "f65": ((65, 1, 64), 128.0, 64, 64, 32, 0.0, np.inf),     # one row past a 64-row tile
    "g": ((1, 2, 4096), 1024.0, 2048, None, 1024, 0.5, 100.0),  # the envelope's largest table, K = 200
    "h": ((2, 60000), 250.0, 256, None, 128, 0.0, np.inf),    # few rows, S = 467: the segment split and its reduce
}
EXPECT = {"a": (3, 129), "b": (7, 45), "c": (4, 19), "d": (1, 128), "e": (1, 1), "f17": (1, 33), "f65": (1, 33),
          "g": (3, 200), "h": (467, 129)}                       # (S, K)
ASYM_TAPS = np.linspace(0.2, 1.0, 200) ** 2 + 0.05 * np.sin(np.arange(200))   # case b, an asymmetric window


def make_data(shape, sfreq, seed=0):
    """standard_normal + 2 sin(2 pi 10 t) + a per-row offset cycling through 0, 50, -200 (float64)."""
    rng = np.random.default_rng(seed + int(np.prod(shape)))
    T = shape[-1]
    rows = int(np.prod(shape[:-1]))
    x = rng.standard_normal((rows, T)) + 2.0 * np.sin(2.0 * np.pi * 10.0 * np.arange(T) / sfreq)
    x += np.array([0.0, 50.0, -200.0])[np.arange(rows) % 3][:, None]
    return x.reshape(shape)


def scipy_window(window):
    return window if isinstance(window, str) else np.asarray(window)


def ref_welch(x, sfreq, n_fft, n_per_seg, n_overlap, fmin, fmax, window="hamming", remove_dc=True, average="mean"):
    """scipy.signal.welch under MNE's segment rules -> (psds [..., K], freqs [K], S)."""
    T = x.shape[-1]
    nps = n_fft if n_per_seg is None or n_per_seg > n_fft else n_per_seg
    nps = min(nps, T)
    f, p = ss.welch(x, sfreq, window=scipy_window(window), nperseg=nps, noverlap=n_overlap, nfft=n_fft,
                    detrend="constant" if remove_dc else False, scaling="density", average=average)
    mask = (f >= fmin) & (f <= fmax)
    seg_times = ss.spectrogram(x.reshape(-1, T)[0], sfreq, window=scipy_window(window), nperseg=nps,
                               noverlap=n_overlap, nfft=n_fft)[1]
    return p[..., mask], f[mask], seg_times.size


def ref_spectrogram(x, sfreq, n_fft, n_per_seg, n_overlap, fmin, fmax, window="hamming", remove_dc=True):
    T = x.shape[-1]
    nps = min(n_fft if n_per_seg is None or n_per_seg > n_fft else n_per_seg, T)
    f, _, p = ss.spectrogram(x, sfreq, window=scipy_window(window), nperseg=nps, noverlap=n_overlap, nfft=n_fft,
                             detrend="constant" if remove_dc else False, scaling="density", mode="psd")
    mask = (f >= fmin) & (f <= fmax)
    return p[..., mask, :]


def design_product(psd, x, sfreq, d, remove_dc):
    """The dense product the kernel computes, in NumPy float64 from the design's own window, bins and scale."""
    rows = x.reshape(-1, x.shape[-1])
    idx = np.arange(d.n_segments)[:, None] * d.step + np.arange(d.n_per_seg)[None, :]
    segs = rows[:, idx]                                            # [rows, S, n_per_seg]
    if remove_dc:
        segs = segs - segs.mean(-1, keepdims=True)
    k, t = np.arange(d.k_lo, d.k_hi + 1), np.arange(d.n_per_seg)
    ang = 2.0 * np.pi * ((k[:, None] * t[None, :]) % d.n_fft) / d.n_fft
    re, im = segs @ (d.window * np.cos(ang)).T, segs @ (d.window * np.sin(ang)).T
    return ((re * re + im * im) * d.scale).mean(1).reshape(x.shape[:-1] + (k.size,))


@pytest.fixture(scope="module")
def psd():
    from isd_amd import psd
    return psd


@pytest.mark.parametrize("remove_dc", [True, False])
@pytest.mark.parametrize("window", ["hamming", "hann"])
@pytest.mark.parametrize("case", sorted(PARAMS))
def test_welch_design_against_scipy(psd, case, window, remove_dc):
    shape, sfreq, n_fft, n_per_seg, n_overlap, fmin, fmax = PARAMS[case]
    if case == "h":
        shape = (2, 6000)                                          # the same design on a tenth of the samples
    x = make_data(shape, sfreq)
    d = psd.welch_design(sfreq, shape[-1], fmin, fmax, n_fft, n_overlap, n_per_seg, window)
    ref, f, S = ref_welch(x, sfreq, n_fft, n_per_seg, n_overlap, fmin, fmax, window, remove_dc)
    assert d.n_segments == S and d.step == d.n_per_seg - d.n_overlap
    if case != "h":
        assert (d.n_segments, d.k_hi - d.k_lo + 1) == EXPECT[case]
    assert d.freqs.dtype == np.float64 and np.array_equal(d.freqs, f)
    assert d.window.shape == (d.n_per_seg,) and d.scale.shape == f.shape
    got = design_product(psd, x, sfreq, d, remove_dc)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"case {case} {window} remove_dc={remove_dc}: {err:.2e}")
    assert err < 1e-12


def test_explicit_taps_against_scipy(psd):
    shape, sfreq, n_fft, n_per_seg, n_overlap, fmin, fmax = PARAMS["b"]
    x = make_data(shape, sfreq)
    d = psd.welch_design(sfreq, shape[-1], fmin, fmax, n_fft, n_overlap, n_per_seg, ASYM_TAPS)
    ref, f, _ = ref_welch(x, sfreq, n_fft, n_per_seg, n_overlap, fmin, fmax, ASYM_TAPS)
    assert np.array_equal(d.freqs, f) and np.array_equal(d.window, ASYM_TAPS)
    assert np.abs(design_product(psd, x, sfreq, d, True) - ref).max() / np.abs(ref).max() < 1e-12
    with pytest.raises(ValueError):
        psd.welch_design(sfreq, shape[-1], fmin, fmax, n_fft, n_overlap, n_per_seg, ASYM_TAPS[:-1])
    with pytest.raises(ValueError):
        psd.welch_design(sfreq, shape[-1], fmin, fmax, n_fft, n_overlap, n_per_seg, np.zeros(200))


def test_segment_resolution_rules(psd):
    d = psd.welch_design(250, 795, n_fft=256)
    assert (d.n_per_seg, d.step, d.n_segments) == (256, 256, 3)    # n_per_seg=None means n_fft
    d = psd.welch_design(250, 795, n_fft=256, n_per_seg=400, n_overlap=56)
    assert (d.n_per_seg, d.step, d.n_segments) == (256, 200, 3)    # clamped to n_fft
    d = psd.welch_design(250, 100, n_fft=256, n_per_seg=128)
    assert (d.n_per_seg, d.n_segments) == (100, 1)                 # clamped to the samples
    d = psd.welch_design(250, 1000, fmin=10, fmax=10, n_fft=250)
    assert (d.k_lo, d.k_hi) == (10, 10) and d.freqs.tolist() == [10.0]   # both ends inclusive
    d = psd.welch_design(250, 512, n_fft=256)
    assert d.scale[0] * 2 == d.scale[1] == d.scale[-2] == 2 * d.scale[-1]      # DC and Nyquist count once
    d = psd.welch_design(250, 512, n_fft=255)
    assert d.k_hi == 127 and d.scale[0] * 2 == d.scale[1] == d.scale[-1]       # odd n_fft: no Nyquist bin


def test_argument_errors(psd):
    with pytest.raises(ValueError, match="n_fft"):
        psd.welch_design(250, 200, n_fft=256)
    with pytest.raises(ValueError, match="n_overlap"):
        psd.welch_design(250, 795, n_fft=256, n_per_seg=128, n_overlap=128)
    with pytest.raises(ValueError, match="n_overlap"):
        psd.welch_design(250, 100, n_fft=256, n_per_seg=200, n_overlap=100)    # n_per_seg was clamped to 100
    with pytest.raises(ValueError, match="no frequency bin"):
        psd.welch_design(250, 795, fmin=9.8, fmax=10.7, n_fft=256)
    with pytest.raises(ValueError, match="no frequency bin"):
        psd.welch_design(250, 256, fmin=10, fmax=10.5, n_fft=256)              # 9.766 and 10.742 Hz: nothing between
    with pytest.raises(NotImplementedError):
        psd.welch_design(250, 795, n_fft=256, window="blackman")
    x = np.zeros((2, 795))
    with pytest.raises(NotImplementedError):
        psd.psd_array_welch(x, 250, output="complex")
    with pytest.raises(NotImplementedError):
        psd.psd_array_welch(x, 250, n_fft=4096, n_per_seg=512)
    with pytest.raises(NotImplementedError):
        psd.psd_array_multitaper(x, 250)
    with pytest.raises(ValueError):
        psd.psd_array_welch(x, 250, average="max")
    with pytest.raises(TypeError):
        psd.psd_array_welch(np.zeros((2, 795), dtype=np.int32), 250)


@pytest.mark.parametrize("n", [1, 2, 7, 100, 200, 255, 256])
def test_periodic_windows_equal_scipy(psd, n):
    for name in ("hamming", "hann"):
        w = psd.periodic_window(name, n)
        assert w.dtype == np.float64 and np.abs(w - ss.get_window(name, n)).max() <= 1e-15


def test_median_bias_equals_scipy(psd):
    from scipy.signal._spectral_py import _median_bias
    for S in range(1, 13):
        assert psd.median_bias(S) == _median_bias(S)
    assert psd.median_bias(7) == 0.7595238095238095


def test_band_power_hand_sum(psd):
    import torch
    freqs = np.arange(0.0, 11.0) * 0.5                              # 0, 0.5, ... 5 Hz
    p = np.arange(1.0, 23.0).reshape(2, 11)
    bands = (("lo", 0.5, 2.0), ("hi", 2.0, 4.0), ("none", 7.0, 9.0))
    want = np.stack([p[:, 1:5].sum(-1) * 0.5, p[:, 4:9].sum(-1) * 0.5, np.zeros(2)], axis=-1)   # edges inclusive
    got = psd.band_power(p, freqs, bands)
    assert got.shape == (2, 3) and np.array_equal(got, want)
    rel = psd.band_power(p, freqs, bands, relative=True)
    assert np.allclose(rel, want / (p.sum(-1, keepdims=True) * 0.5), rtol=1e-15, atol=0)
    gt = psd.band_power(torch.as_tensor(p), freqs, bands, relative=True)
    assert isinstance(gt, torch.Tensor) and np.array_equal(gt.numpy(), rel)
    assert psd.band_power(p.reshape(1, 2, 11), freqs).shape == (1, 2, 5)      # BANDS_5 by default
    with pytest.raises(ValueError):
        psd.band_power(p, freqs[:-1])


def test_import_does_not_load_the_library():
    code = ("import isd_amd, isd_amd.psd, isd_amd._lib as L; "
            "assert isd_amd.psd_array_welch is isd_amd.psd.psd_array_welch; "
            "isd_amd.psd.welch_design(250, 795); assert L._lib is None; print('ok')")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
