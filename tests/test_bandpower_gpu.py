"""``Stft.bandpower`` (isd_stft_bandpower) on every route, mode and band shape against the fp64 reference of
bandpower_ref.py.  Every case draws fp32 standard-normal rows, asserts the kernel instance through
``isd_stft_bandpower_last_path`` (family + 16 * instance) and runs power, magnitude and log power.

Instance -> case (tables in bandpower_ref.py); the reporter's value is asserted in each:

    bandpower_direct_kernel<false, false>   1   direct-t512_c3_ragged, t481 .. t1      power, logpower
    bandpower_direct_kernel<false, true>   17   direct-t512_c1_full, t512_c5_full      power, logpower
    bandpower_direct_kernel<true, false>    1   direct-t512_c3_ragged, t481 .. t1      magnitude
    bandpower_direct_kernel<true, true>    17   direct-t512_c1_full, t512_c5_full      magnitude
    bandpower_blocksum_kernel<64, 4>       66   blocksum-h64_kb4, h64_single_bins
    bandpower_blocksum_kernel<64, 5>       82   blocksum-h64_kb5
    bandpower_blocksum_kernel<64, 6>       98   blocksum-h64_kb6
    bandpower_blocksum_kernel<64, 8>      130   blocksum-h64_kb8, h64_kb8_j65
    bandpower_blocksum_kernel<32, 4>       66   blocksum-h32_kb4, h32_single_bins
    bandpower_blocksum_kernel<32, 5>       82   blocksum-h32_kb5
    bandpower_blocksum_kernel<32, 6>       98   blocksum-h32_kb6
    bandpower_blocksum_kernel<32, 8>      130   blocksum-h32_kb8
    stft_kernel<1>                          3   fft-*, fft-*_shared, fallback-*

Bounds (none taken from the kernels under test):
  power, magnitude   |got - ref| <= 2e-5 max(ref) per call, the bound of test_overlapped_frames_bandpower_vs_oracle;
                     exactly 0.0 where the reference power is exactly 0 (empty bands, frames that hold no sample or
                     only one under the window's zero)
  log power          |got - ref| <= 1e-4 max(1, |ref|) everywhere (north-star gate); the plain 1e-4 where the reference
                     power is above the row median / 1e4 (test_bandpower_cpu.py caps what that mask leaves out);
                     log(eps) within 1e-4 where the power is 0
"""
import numpy as np
import pytest
import torch

import bandpower_ref as bref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def isd():
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd


def last_path():
    from isd_amd import _lib
    return _lib.lib().isd_stft_bandpower_last_path()


def run_case(isd, case, mode):
    """(values as float64, reporter's value) of one call."""
    n, nov, T, B, C, bins, shared = bref.CASES[case]
    y = torch.from_numpy(bref.make(case).copy()).cuda()
    st = isd.Stft(T, n, nov)
    got = st.bandpower(y, bins, mode=mode, eps=bref.EPS, shared_signal=shared)
    assert got.shape == (B, len(bins), C, st.n_frames) and got.dtype == torch.float32
    path = last_path()
    return got.cpu().numpy().astype(np.float64), path


def check_case(case, mode, got):
    ref, power = bref.reference(case)
    ref = ref[mode]
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = np.abs(got - ref)
    zero = power == 0
    if mode == "logpower":
        loud = bref.loud_mask(power)
        gate = err / np.maximum(1.0, np.abs(ref))
        print(f"BANDPOWER {case} {mode}: max err {err.max():.3e}, loud {err[loud].max():.3e}, "
              f"relative gate {gate.max():.3e}, quiet values {int((~loud & ~zero).sum())}, zero {int(zero.sum())}")
        assert (gate <= 1e-4).all()
        assert err[loud].max() <= 1e-4
        assert (err[zero] <= 1e-4).all()
    else:
        print(f"BANDPOWER {case} {mode}: max err / max ref {err.max() / ref.max():.3e}, zero {int(zero.sum())}")
        assert (got[zero] == 0.0).all()
        assert err.max() <= 2e-5 * ref.max()


@pytest.mark.parametrize("mode", bref.MODES)
@pytest.mark.parametrize("case", bref.case_names("direct"))
def test_direct_dft(isd, case, mode):
    """bandpower_direct_kernel<MAG, FULL>: DC, Nyquist, single-bin, empty and full-range bands in one call, 1 / 3 / 4 /
    5 channels (waves whose rows belong to up to four bands, ragged last quads), rows from 1 to 512 samples."""
    n, nov, T, B, C, bins, shared = bref.CASES[case]
    got, path = run_case(isd, case, mode)
    full = T == 512 and (B * len(bins) * C) % 4 == 0
    assert path == bref.DIRECT + 16 * int(full), (case, path)
    check_case(case, mode, got)


@pytest.mark.parametrize("mode", bref.MODES)
@pytest.mark.parametrize("case", bref.case_names("blocksum"))
def test_block_sums(isd, case, mode):
    """bandpower_blocksum_kernel<hop, KB>, one case per instance and more: 4 / 8 / 16 / 64 blocks per frame, J = 65,
    ragged rows, rows shorter than a block, bands beside DC and Nyquist, all-single-bin band sets."""
    n, nov, T, B, C, bins, shared = bref.CASES[case]
    got, path = run_case(isd, case, mode)
    fam, kb = bref.expected_path(n, nov, T, bins)
    assert fam == bref.BLOCKSUM and path == bref.BLOCKSUM + 16 * kb, (case, path)
    check_case(case, mode, got)


@pytest.mark.parametrize("mode", bref.MODES)
@pytest.mark.parametrize("case", bref.case_names("fallback"))
def test_block_sum_plans_fall_back_to_fft(isd, case, mode):
    """On a plan that has a block-sum table, one band of seven bins, or one that touches bin 0 or n/2, sends the call
    to the FFT kernel, and the values are still right."""
    got, path = run_case(isd, case, mode)
    assert path == bref.FFT, (case, path)
    check_case(case, mode, got)


@pytest.mark.parametrize("mode", bref.MODES)
@pytest.mark.parametrize("case", bref.case_names("fft"))
def test_fft_band_reduction(isd, case, mode):
    """stft_kernel<1>, per-band and shared input: nperseg 8 .. 2048 with hops that do not divide it, dead frames in
    the last workgroup, empty / full-range / DC / Nyquist bands, 64 bands on 4 threads per frame, and nperseg 64 / hop
    32 just past the direct kernel's T <= 512."""
    got, path = run_case(isd, case, mode)
    assert path == bref.FFT, (case, path)
    check_case(case, mode, got)


def test_reporter_is_per_call(isd):
    """The value follows the last call, whatever ran before it, and a call without a launch leaves it."""
    seq = ["direct-t512_c1_full", "fft-n8", "blocksum-h32_kb6", "direct-t31_c1", "blocksum-h64_kb4", "fallback-h64_kb4_dc"]
    want = [17, 3, 98, 1, 66, 3]
    for case, w in zip(seq, want):
        assert run_case(isd, case, "power")[1] == w, case
    st = isd.Stft(512, 64, 32)
    out = st.bandpower(torch.empty((0, 2, 3, 512), device="cuda"), [(1, 2), (3, 4)])
    assert out.shape == (0, 2, 3, 17) and last_path() == 3
