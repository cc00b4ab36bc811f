"""The fp64 band-power reference of test_bandpower_gpu.py, checked without a GPU: its STFT against scipy's own on
every plan of the case tables, the loud-value mask's cap on every case, and the tables' coverage of the routes."""
import numpy as np
import pytest

import bandpower_ref as bref
from oracle import dsp as odsp


@pytest.mark.parametrize("T,nperseg,noverlap", bref.plans())
def test_stft_restatement_matches_scipy(T, nperseg, noverlap):
    """oracle.dsp.stft in fp64 against scipy.signal.stft with the legacy defaults the plan restates (periodic Hann,
    boundary='zeros', padded=True, scaling='spectrum'): frame count, bin count, Z within 1e-12 of its largest magnitude.
    scipy shortens the window of a row shorter than nperseg, which the plan does not: such a row goes to scipy with
    zeros appended up to nperseg -- the samples the zero boundary supplies anyway -- and the plan's J frames are the
    first J of scipy's; the frame count is then checked against the padded-length formula alone."""
    import scipy.signal as ss
    x = np.random.default_rng(T + nperseg).standard_normal((3, T))
    _, _, Z = odsp.stft(x, 1.0, nperseg, noverlap)
    J, _ = odsp.stft_frames(T, nperseg, noverlap)
    assert Z.shape == (3, nperseg // 2 + 1, J) and Z.dtype == np.complex128
    xs = x if T >= nperseg else np.concatenate([x, np.zeros((3, nperseg - T))], axis=-1)
    _, _, ref = ss.stft(xs, fs=1.0, window="hann", nperseg=nperseg, noverlap=noverlap, boundary="zeros", padded=True,
                        scaling="spectrum")
    assert ref.shape[-2] == Z.shape[-2]
    if T >= nperseg:
        assert ref.shape[-1] == J
    else:
        assert ref.shape[-1] >= J
    assert np.abs(Z - ref[..., :J]).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("case", list(bref.CASES))
def test_loud_mask_cap_and_zero_power(case):
    """The plain 1e-4 log-domain bound covers the values whose power is above the row median / 1e4.  That mask may
    leave out at most 10 % of a case's nonzero-power values; a case whose inputs break the cap is changed, not masked
    further.  Exactly-zero power is what an empty band gives, and a frame that holds no sample or only one under the
    window's zero."""
    n, nov, T, B, C, bins, shared = bref.CASES[case]
    ref, power = bref.reference(case)
    J, _ = odsp.stft_frames(T, n, nov)
    assert power.shape == (B, len(bins), C, J) and np.isfinite(ref["logpower"]).all()
    nonzero = power > 0
    left_out = nonzero & ~bref.loud_mask(power)
    assert left_out.sum() <= 0.1 * nonzero.sum(), (case, int(left_out.sum()), int(nonzero.sum()))
    for b, (lo, hi) in enumerate(bins):
        assert (hi < lo) == (not nonzero[:, b].any()), (case, b)
    assert (ref["power"][~nonzero] == 0).all() and (ref["magnitude"][~nonzero] == 0).all()
    np.testing.assert_allclose(ref["logpower"][~nonzero], np.log(bref.EPS), rtol=0, atol=1e-12)
    # log power, power and magnitude of one bin say the same thing
    np.testing.assert_allclose(np.exp(ref["logpower"]) - bref.EPS, power, rtol=1e-9, atol=1e-18)
    for b, (lo, hi) in enumerate(bins):
        if hi == lo:
            np.testing.assert_allclose(ref["magnitude"][:, b] ** 2, power[:, b], rtol=1e-12, atol=0)


def test_zero_power_frames_are_where_the_window_says():
    """The last frame of a nperseg 64 / hop 32 row of 32 m + 1 samples holds one sample under the window's zero."""
    for case in ("direct-t481_c3", "direct-t33_c3", "direct-t1_c4", "fft-n64_t513"):
        _, power = bref.reference(case)
        bins = bref.CASES[case][5]
        live = [b for b, (lo, hi) in enumerate(bins) if hi >= lo]
        assert (power[:, live, :, -1] == 0).all() and (power[:, live, :, :-1] > 0).all(), case


def test_case_tables_cover_every_route():
    """Every block-sum instance <hop, KB> and blocks-per-frame count has a case; the fall-back cases sit on plans
    that have a block-sum table and still go to the FFT kernel; the direct cases hold both FULL and ragged shapes."""
    seen, nblks = set(), set()
    for name in bref.case_names("blocksum"):
        n, nov, T, B, C, bins, shared = bref.CASES[name]
        fam, kb = bref.expected_path(n, nov, T, bins)
        assert fam == bref.BLOCKSUM, name
        seen.add((n - nov, kb))
        nblks.add(n // (n - nov))
    assert seen == {(h, kb) for h in (32, 64) for kb in (4, 5, 6, 8)}
    assert nblks >= {4, 8, 16, 64}
    for name in bref.case_names("fallback"):
        n, nov, T, B, C, bins, shared = bref.CASES[name]
        assert bref.expected_path(n, nov, T, bins) == (bref.FFT, 0), name
        assert bref.expected_path(n, nov, T, [(1, 1)])[0] == bref.BLOCKSUM, name
    for name in bref.case_names("fft"):
        n, nov, T, B, C, bins, shared = bref.CASES[name]
        assert bref.expected_path(n, nov, T, bins, shared) == (bref.FFT, 0), name
    full = {(T == 512 and (B * len(bins) * C) % 4 == 0) for T, B, C, bins in bref.DIRECT_CASES.values()}
    assert full == {True, False}
    assert {C for _, _, C, _ in bref.DIRECT_CASES.values()} == {1, 3, 4, 5}
    assert {T for T, _, _, _ in bref.DIRECT_CASES.values()} == {512, 481, 480, 250, 33, 31, 1}
