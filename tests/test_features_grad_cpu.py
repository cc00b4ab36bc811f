"""Spec S restated in float64 torch (differentiable: the reference of the GPU input-gradient tests), held against the
oracle on the G3 shapes; and the argument checks of isd_features_backward, which need no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import dsp as odsp

MODES = ("logpower", "power", "magnitude")


def band_impulse_responses(fs, bands, T, order=4):
    """[nb, T] float64: each band's Butterworth cascade (oracle.dsp) driven by a unit impulse, truncated to T."""
    imp = np.zeros((1, T))
    imp[0, 0] = 1.0
    return np.stack([odsp.sosfilt(odsp.butter_bandpass_sos(order, lo, hi, fs), imp)[0]
                     for lo, hi in odsp.band_edges(bands)])


def spec_s_reference(x, fs, bands, nperseg=64, noverlap=None, eps=1e-10, mode="logpower", order=4, h=None):
    """x float64 torch [B, C, T] -> (features [B, nb, C, J], filtered [B, nb, C, T]), both float64 and differentiable.

    filter: causal FFT convolution with the band's impulse response (zero initial state, truncated to T); STFT: explicit
    zero extension by nperseg/2, zero padding to whole frames, periodic Hann, rfft, scaling 1/sum(w); band means over
    the inclusive bins of global_shap_analysis.py:151-156; logpower / power / magnitude."""
    B, Cc, T = x.shape
    noverlap = nperseg // 2 if noverlap is None else noverlap
    hop, half = nperseg - noverlap, nperseg // 2
    J, L = odsp.stft_frames(T, nperseg, noverlap)
    if h is None:
        h = band_impulse_responses(fs, bands, T, order)
    nfft = 1 << int(np.ceil(np.log2(2 * T)))
    Hf = torch.fft.rfft(torch.as_tensor(h, dtype=torch.float64), nfft)           # [nb, nfft/2+1]
    y = torch.fft.irfft(torch.fft.rfft(x, nfft)[:, None] * Hf[None, :, None], nfft)[..., :T]   # [B, nb, C, T]
    win = torch.as_tensor(odsp.hann_periodic(nperseg), dtype=torch.float64)
    scale = 1.0 / win.sum()
    xp = torch.nn.functional.pad(y, (half, L - half - T))
    Z = torch.fft.rfft(xp.unfold(-1, nperseg, hop) * win, dim=-1) * scale        # [B, nb, C, J, nfreq]
    feats = []
    for b, (klo, khi) in enumerate(odsp.band_bins(fs, nperseg, bands)):
        if khi < klo:
            v = torch.zeros((B, Cc, J), dtype=torch.float64)
            feats.append(torch.log(v + eps) if mode == "logpower" else v)
            continue
        Zb = Z[:, b, :, :, klo:khi + 1]
        if mode == "magnitude":
            feats.append(Zb.abs().mean(-1))
        else:
            P = (Zb.real ** 2 + Zb.imag ** 2).mean(-1)
            feats.append(torch.log(P + eps) if mode == "logpower" else P)
    return torch.stack(feats, 1), y


def _g3(tag):
    g = load_golden("g3_features.npz")
    B, Cc, T, fs, nperseg, nov, nb = g[f"{tag}_cfg"]
    x = g[f"{tag}_x"] if f"{tag}_x" in g.files else \
        np.random.default_rng(3).standard_normal((int(B), int(Cc), int(T))).astype(np.float32)
    return x, float(fs), int(nperseg), int(nov)


G3 = [("c1", odsp.BANDS_5), ("c2", odsp.BANDS_9), ("c5", odsp.BANDS_40[:6]), ("c800", odsp.BANDS_9)]


@pytest.mark.parametrize("tag,bands", G3)
def test_reference_matches_oracle_on_g3_shapes(tag, bands):
    x, fs, nperseg, nov = _g3(tag)
    x = x[:2, :4]                                                  # a few rows: the oracle's sosfilt is a Python loop
    feat_o, filt_o = odsp.extract_features(x, fs=fs, bands=bands, nperseg=nperseg, noverlap=nov, return_filtered=True)
    xt = torch.as_tensor(x, dtype=torch.float64)
    feat, y = spec_s_reference(xt, fs, bands, nperseg, nov)
    y = y.numpy()
    assert np.abs(y - filt_o).max() <= 1e-10 * np.abs(filt_o).max()
    feat = feat.numpy()
    assert feat.shape == feat_o.shape
    # the oracle's features are float64 rounded once to float32: agreement to that rounding
    assert (np.abs(feat - feat_o) <= 1.2e-7 * np.abs(feat_o) + 1e-9).all()
    mag, _ = spec_s_reference(xt, fs, bands, nperseg, nov, mode="magnitude")
    _, _, Z = odsp.stft(filt_o, fs, nperseg, nov)                  # [B, nb, C, nfreq, J]
    ref = odsp.band_magnitude(Z, fs, nperseg, bands)               # [B, nb(signal), C, nb(bins), J]
    ref = np.stack([ref[:, b, :, b] for b in range(len(bands))], 1)
    assert np.abs(mag.numpy() - ref).max() <= 1e-10 * np.abs(ref).max()
    power, _ = spec_s_reference(xt, fs, bands, nperseg, nov, mode="power")
    assert np.allclose(np.log(power.numpy() + 1e-10), feat, rtol=0, atol=1e-12)


def test_reference_is_differentiable_and_causal():
    x = torch.randn(1, 2, 200, dtype=torch.float64, requires_grad=True)
    feat, _ = spec_s_reference(x, 256.0, odsp.BANDS_9[:2])
    g = torch.zeros_like(feat)
    g[..., 3] = 1.0                                                # frame 3 covers samples [3*32 - 32, 3*32 + 32)
    dx, = torch.autograd.grad(feat, x, g)
    assert dx[..., 128:].abs().max() < 1e-12 * dx.abs().max()
    assert dx[..., 127].abs().max() > 0


# ---------------------------------------------------------------- the C ABI without a GPU
@pytest.fixture(scope="module")
def lib():
    from isd_amd import _lib
    return _lib


def _call(lib, plan, mode=2, B=1):
    L = lib.lib()
    klo, khi = lib.int_array([2]), lib.int_array([3])
    rc = L.isd_features_backward(plan, plan, None, None, None, None, B, 4, klo, khi, mode, 1e-10, None)
    return rc, L.isd_last_error().decode()


def test_backward_symbols_are_declared(lib):
    assert "isd_features_backward" in lib.SIGNATURES and "isd_features_backward_workspace_bytes" in lib.SIGNATURES


@pytest.mark.parametrize("case,kw,needle", [("null plan", {}, "null plan"),
                                            ("bad mode", {"mode": 7}, "bad mode"),
                                            ("negative B", {"B": -1}, "bad shape")])
def test_backward_rejects_bad_arguments(lib, case, kw, needle):
    rc, msg = _call(lib, None, **kw)
    assert rc == lib.ISD_ERR_INVALID, case
    assert "isd_features_backward" in msg and needle in msg, msg


def test_backward_workspace_query_rejects_null_plan(lib):
    L = lib.lib()
    n = L.isd_features_backward_workspace_bytes(None, None, 4, 4, lib.int_array([2]), lib.int_array([3]))
    assert n == lib.ISD_ERR_INVALID and "null plan" in L.isd_last_error().decode()
