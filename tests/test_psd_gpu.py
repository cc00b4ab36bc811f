"""isd_amd.psd_array_welch on the GPU against scipy.signal.welch / spectrogram (float64), cases of test_psd_cpu.PARAMS.

Data: standard_normal + 2 sin(2 pi 10 t) + a per-row offset cycling through 0, 50, -200.  For float32 the reference is
scipy on the float32-rounded input widened to float64.  Bounds: the largest absolute error of a call over the
reference's largest value below TOL64 = 1e-12 / TOL32 = 1e-5 (test_fir_gpu.py, test_csp_gpu.py); in fp64 also a
per-bin relative error below 1e-10 over the bins whose reference exceeds 1e-6 of their row's maximum.

That mask must not empty the per-bin check.  With remove_dc=True it keeps >= 99.9 % of every case's bins and the test
asserts >= 90 % over all rows.  With remove_dc=False the rows that carry an offset of 50 or -200 have a DC bin 1e7 to
3e9 times their noise floor, so in scipy's own output the mask keeps 67 % (case a), 72 % (d), 82 % (f), 83 % (g) of a
case's bins whatever the kernel does: there the >= 90 % is asserted over the rows without an offset, and the per-bin
bound still holds on every kept bin of every row.

Case e: the bins of n_fft 256 at 250 Hz lie 0.977 Hz apart and none falls in 10 .. 10.5 Hz, so the one-bin case
takes 9.5 .. 10.5 Hz (bin 10 at 9.766 Hz); the empty band is an error, tested in test_psd_cpu.py.

Observed on an MI355X (worst over the cases; each test prints its own figures):
  mean, fp64     3.9e-15 (f65)             per bin 6.6e-12 (f65, remove_dc=True), dynamic range up to 3.5e9
  mean, fp32     1.7e-6  (g, n_fft 2048);  with the offset rows at n_fft 256: 4.4e-7 (b, remove_dc=False)
  hann / taps    1.6e-15 / 6.0e-16 fp64,   3.0e-7 / 1.4e-7 fp32
  average=None   2.5e-15 fp64 (h), per bin 8.0e-12 (a);  1.1e-6 fp32 (h)
  median         1.6e-15 fp64,  5.3e-7 fp32 (h, S = 467)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_psd_cpu import ASYM_TAPS, PARAMS, make_data, ref_spectrogram, ref_welch

pytestmark = pytest.mark.gpu

TOL64, TOL32 = 1e-12, 1e-5
BIN_TOL64, BIN_FLOOR = 1e-10, 1e-6
DTYPES = [(torch.float64, TOL64), (torch.float32, TOL32)]
_REFS = {}


@pytest.fixture(scope="module")
def isd():
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd


def case_data(case, dtype, T=None):
    """(float64 ndarray the reference sees, CUDA tensor of `dtype`): for float32 the rounded input widened back."""
    shape, sfreq = PARAMS[case][:2]
    if T is not None:
        shape = shape[:-1] + (T,)
    key = ("x", case, shape, dtype)
    if key not in _REFS:
        x = make_data(shape, sfreq)
        if dtype == torch.float32:
            x = x.astype(np.float32).astype(np.float64)
        x.setflags(write=False)
        _REFS[key] = x
    x = _REFS[key]
    return x, torch.tensor(x, dtype=dtype).cuda()


def reference(kind, case, dtype, window="hamming", remove_dc=True, T=None):
    wkey = window if isinstance(window, str) else "taps"
    key = (kind, case, dtype, wkey, remove_dc, T)
    if key not in _REFS:
        x, _ = case_data(case, dtype, T)
        args = PARAMS[case][1:]
        if kind == "segments":
            ref = ref_spectrogram(x, *args, window, remove_dc)
        else:
            ref = ref_welch(x, *args, window, remove_dc, average=kind)[0]
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def call(isd, x, case, **kw):
    _, sfreq, n_fft, n_per_seg, n_overlap, fmin, fmax = PARAMS[case]
    return isd.psd_array_welch(x, sfreq, fmin, fmax, n_fft, n_overlap, n_per_seg, **kw)


def _err(got, ref):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())


def fenced(x, dtype, shift):
    """x as a contiguous view into a larger NaN-filled device buffer: NaN directly before its first and after its
    last row.  shift = 1 moves the block off its 16-byte alignment."""
    pad = 64
    buf = torch.full((x.size + 2 * pad + shift,), float("nan"), dtype=dtype, device="cuda")
    view = buf[pad + shift:pad + shift + x.size].view(x.shape)
    view.copy_(torch.tensor(x))
    return buf, view


# ------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("remove_dc", [True, False])
@pytest.mark.parametrize("case", sorted(PARAMS))
def test_mean_matches_scipy(isd, case, remove_dc):
    for dtype, tol in DTYPES:
        x, xd = case_data(case, dtype)
        ref = reference("mean", case, dtype, "hamming", remove_dc)
        got, freqs = call(isd, xd, case, remove_dc=remove_dc)
        assert got.is_cuda and got.dtype == dtype and tuple(got.shape) == ref.shape
        assert isinstance(freqs, np.ndarray) and freqs.dtype == np.float64 and freqs.shape == (ref.shape[-1],)
        err = _err(got, ref)
        print(f"case {case} {str(dtype)[6:]} remove_dc={remove_dc}: max|err|/max|ref| = {err:.2e}")
        assert err < tol
        if dtype == torch.float64:
            r = ref.reshape(-1, ref.shape[-1])
            g = got.cpu().numpy().reshape(r.shape)
            mask = r > BIN_FLOOR * r.max(-1, keepdims=True)
            kept = mask.mean() if remove_dc else mask[::3].mean()      # rows 0, 3, ... carry no offset
            rel = float((np.abs(g - r)[mask] / r[mask]).max())
            print(f"case {case} float64 remove_dc={remove_dc}: per-bin rel = {rel:.2e} over {mask.mean():.1%} of the "
                  f"bins, dynamic range {r.max() / r[mask].min():.1e}")
            assert kept >= 0.9
            assert rel < BIN_TOL64


@pytest.mark.parametrize("window", ["hann", "taps"])
def test_other_windows_case_b(isd, window):
    w = ASYM_TAPS if window == "taps" else window
    for dtype, tol in DTYPES:
        _, xd = case_data("b", dtype)
        ref = reference("mean", "b", dtype, w, True)
        err = _err(call(isd, xd, "b", window=w)[0], ref)
        print(f"case b {window} {str(dtype)[6:]}: {err:.2e}")
        assert err < tol


@pytest.mark.parametrize("case", ["a", "b", "c", "h"])
def test_per_segment_matches_spectrogram(isd, case):
    for dtype, tol in DTYPES:
        _, xd = case_data(case, dtype)
        ref = reference("segments", case, dtype)
        got, _ = call(isd, xd, case, average=None)
        assert tuple(got.shape) == ref.shape and got.dtype == dtype        # [..., K, S]
        err = _err(got, ref)
        print(f"case {case} average=None {str(dtype)[6:]}: {err:.2e}")
        assert err < tol
        if dtype == torch.float64:
            mask = ref > BIN_FLOOR * ref.max((-2, -1), keepdims=True)
            rel = float((np.abs(got.cpu().numpy() - ref)[mask] / ref[mask]).max())
            print(f"case {case} average=None float64: per-bin rel = {rel:.2e} over {mask.mean():.1%}")
            assert mask.mean() >= 0.9 and rel < BIN_TOL64


@pytest.mark.parametrize("case,T", [("b", None), ("h", None), ("h", 60128)])     # S = 7, 467, 468
def test_median_matches_scipy(isd, case, T):
    for dtype, tol in DTYPES:
        _, xd = case_data(case, dtype, T)
        ref = reference("median", case, dtype, T=T)
        got, _ = call(isd, xd, case, average="median")
        assert tuple(got.shape) == ref.shape and got.dtype == dtype
        err = _err(got, ref)
        print(f"case {case} T={T} average='median' {str(dtype)[6:]}: {err:.2e}")
        assert err < tol


# ------------------------------------------------------------------------------------- no read outside the data
@pytest.mark.parametrize("case", ["a", "b", "c", "e", "f17", "g", "h"])
def test_reads_nothing_outside_x(isd, case):
    for dtype, _ in DTYPES:
        x, xd = case_data(case, dtype)
        for average in ("mean", None):
            clean = call(isd, xd, case, average=average)[0]
            for shift in (0, 1):
                buf, view = fenced(x, dtype, shift)
                got = call(isd, view, case, average=average)[0]
                assert torch.isfinite(got).all() and torch.equal(got, clean), (dtype, average, shift)
                assert torch.isnan(buf[:64]).all() and torch.isnan(buf[-64:]).all()


@pytest.mark.parametrize("case", ["a", "c"])
def test_samples_after_the_last_segment_are_not_read(isd, case):
    shape, _, n_fft, n_per_seg, n_overlap = PARAMS[case][:5]
    nps = n_fft if n_per_seg is None else n_per_seg
    used = (shape[-1] - nps) // (nps - n_overlap) * (nps - n_overlap) + nps
    assert used < shape[-1]
    for dtype, _ in DTYPES:
        _, xd = case_data(case, dtype)
        bad = xd.clone()
        bad[..., used:] = float("nan")
        for average in ("mean", None):
            got = call(isd, bad, case, average=average)[0]
            assert torch.isfinite(got).all() and torch.equal(got, call(isd, xd, case, average=average)[0])


# --------------------------------------------------------------------------------------- repeatability, plumbing
@pytest.mark.parametrize("case", ["a", "h"])
def test_two_calls_give_the_same_bits(isd, case):
    for dtype, _ in DTYPES:
        _, xd = case_data(case, dtype)
        assert torch.equal(call(isd, xd, case)[0], call(isd, xd, case)[0])


def test_non_contiguous_and_leading_axes(isd):
    for dtype, _ in DTYPES:
        _, xd = case_data("a", dtype)                                   # (3, 5, 795)
        base = call(isd, xd, "a")[0]
        wide = torch.zeros(3, 5, 2 * 795, dtype=dtype, device="cuda")
        wide[..., ::2] = xd
        view = wide[..., ::2]
        assert not view.is_contiguous() and torch.equal(call(isd, view, "a")[0], base)
        swapped = xd.transpose(0, 1)                                    # (5, 3, 795), non-contiguous
        assert torch.equal(call(isd, swapped, "a")[0], base.transpose(0, 1))
        assert torch.equal(call(isd, xd[1, 2], "a")[0], base[1, 2])                       # (T,)
        assert torch.equal(call(isd, xd[1], "a")[0], base[1])                             # (C, T)
        four = torch.stack([xd, xd.flip(0)])                                              # (2, n, C, T)
        got = call(isd, four, "a")[0]
        assert tuple(got.shape) == (2, 3, 5, 129)
        assert torch.equal(got[0], base) and torch.equal(got[1], base.flip(0))
        seg = call(isd, four, "a", average=None)[0]
        assert tuple(seg.shape) == (2, 3, 5, 129, 3) and torch.equal(seg[1, 0], call(isd, xd[2], "a", average=None)[0])


def test_ndarray_route_is_the_fp64_route(isd):
    x, xd = case_data("b", torch.float64)
    for average in ("mean", "median", None):
        got, freqs = call(isd, x, "b", average=average)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64
        assert np.array_equal(got, call(isd, xd, "b", average=average)[0].cpu().numpy())
    got32 = call(isd, x.astype(np.float32), "b")[0]                      # any float array is computed in fp64
    assert got32.dtype == np.float64
    with pytest.raises(TypeError):
        call(isd, xd.cpu(), "b")


def test_abi_envelope_and_empty_input(isd):
    from isd_amd import _lib
    L = _lib.lib()
    w = _lib.double_array(np.ones(2048))

    def create(n_fft, n_per_seg, n_overlap, k_lo, k_hi):
        h = C.c_void_p()
        rc = L.isd_psd_plan_create(C.byref(h), n_fft, n_per_seg, n_overlap, k_lo, k_hi, w, 250.0, 1)
        if rc == 0:
            L.isd_psd_plan_destroy(h)
        return rc, L.isd_last_error()

    for args, word in (((4096, 256, 0, 0, 10), b"n_fft"), ((256, 128, 128, 0, 10), b"n_overlap"),
                       ((256, 256, 0, 0, 129), b"bins"), ((256, 257, 0, 0, 10), b"n_per_seg")):
        rc, msg = create(*args)
        assert rc == _lib.ISD_ERR_UNSUPPORTED and word in msg, (args, rc, msg)
    assert create(2048, 2048, 2047, 0, 1024)[0] == 0                   # the corners of the envelope
    plan = isd.psd.WelchPlan(256, 256, 0, 0, 128, np.ones(256), 250.0, True)
    assert plan.bins == 129
    assert L.isd_psd_plan_segments(plan._h, 795) == 3 and L.isd_psd_plan_segments(plan._h, 255) == 0
    with pytest.raises(_lib.IsdUnsupported, match="shorter than n_per_seg"):
        plan(torch.zeros(2, 255, device="cuda"))
    for dtype, _ in DTYPES:
        empty = torch.zeros(0, 4, 795, dtype=dtype, device="cuda")
        got, freqs = isd.psd_array_welch(empty, 250)
        assert tuple(got.shape) == (0, 4, 129) and got.dtype == dtype and freqs.shape == (129,)
        assert tuple(isd.psd_array_welch(empty, 250, average=None)[0].shape) == (0, 4, 129, 3)


# ------------------------------------------------------------------------------------------------ with the ICA
def test_ica_sources_band_power_flags_the_40_hz_component(isd):
    rng = np.random.default_rng(5)
    n, Cc, T, m = 6, 8, 400, 4
    t = np.arange(n * T) / 250.0
    src = np.stack([np.sin(2 * np.pi * 40.0 * t + 0.3),                 # the "muscle / line" source
                    np.sign(np.sin(2 * np.pi * 3.0 * t)),               # slow square wave
                    (7.0 * t + 0.1) % 1.0,                              # 7 Hz sawtooth
                    np.convolve(rng.laplace(size=n * T), np.ones(25) / 25, "same")])    # smoothed spikes, < 10 Hz
    src = (src - src.mean(1, keepdims=True)) / src.std(1, keepdims=True)
    X = (rng.standard_normal((Cc, m)) @ src + 0.01 * rng.standard_normal((Cc, n * T)))
    X = np.ascontiguousarray(X.reshape(Cc, n, T).transpose(1, 0, 2))
    xd = torch.as_tensor(X).cuda()
    ica = isd.ICA(m, random_state=0).fit(xd)
    psds, freqs = isd.psd_array_welch(ica.get_sources(xd), 250, n_fft=128)
    assert psds.is_cuda and tuple(psds.shape) == (n, m, 65)
    rel = isd.psd.band_power(psds.mean(0), freqs, relative=True)        # [m, 5 bands]
    gamma = rel[:, 4].cpu().numpy()                                     # 30 - 100 Hz
    print("relative 30-100 Hz power per component:", np.round(gamma, 3))
    assert (gamma > 0.5).sum() == 1
