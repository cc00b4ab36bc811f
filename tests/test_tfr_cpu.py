"""isd_amd.tfr without a GPU and without loading the library: morlet against the NumPy restatement of tests/tfr_ref.py
(values, lengths, norm, conjugate symmetry), every argument error of morlet / cwt / tfr_array_morlet raised before any
GPU use, the output length under decimation, the declarations of the C ABI and the import."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import tfr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_NB = np.arange(4.0, 41.0)                                        # the notebook's 37 frequencies


@pytest.fixture(scope="module")
def tfr():
    from isd_amd import tfr
    return tfr


MORLET_SETS = [
    (250.0, F_NB, 7.0),
    (250.0, F_NB, F_NB / 2.0),
    (250.0, np.array([20.0, 31.0, 40.0, 60.0, 100.0]), 3.0),
    (1024.0, np.array([2.8, 100.0]), 7.0),
    (256.0, np.arange(8.0, 41.0, 2.0), np.arange(8.0, 41.0, 2.0) / 2.0),
]


@pytest.mark.parametrize("zero_mean", [False, True])
@pytest.mark.parametrize("k", range(len(MORLET_SETS)))
def test_morlet_against_the_restatement(tfr, k, zero_mean):
    sfreq, freqs, n_cycles = MORLET_SETS[k]
    got, ref = tfr.morlet(sfreq, freqs, n_cycles, zero_mean=zero_mean), tfr_ref.morlet(sfreq, freqs, n_cycles,
                                                                                       zero_mean=zero_mean)
    assert len(got) == len(ref) == len(freqs)
    worst = 0.0
    for W, R in zip(got, ref):
        assert W.dtype == np.complex128 and W.shape == R.shape and W.shape[0] % 2 == 1
        worst = max(worst, float(np.abs(W - R).max() / np.abs(R).max()))
        assert abs(np.linalg.norm(W) - np.sqrt(2.0)) < 1e-14
        assert np.array_equal(W[::-1], np.conj(W))
    print(f"set {k} zero_mean={zero_mean}: {worst:.2e}")
    assert worst < 1e-15


def test_morlet_sigma_fixes_the_width(tfr):
    got, ref = tfr.morlet(250.0, [10.0, 20.0], 7.0, sigma=10.0), tfr_ref.morlet(250.0, [10.0, 20.0], 7.0, sigma=10.0)
    assert len(got[0]) == len(got[1]) == len(tfr.morlet(250.0, [10.0], 7.0)[0])
    for W, R in zip(got, ref):
        assert np.abs(W - R).max() < 1e-15


def test_pinned_lengths(tfr):
    lens = [len(W) for W in tfr.morlet(250.0, F_NB, 7.0)]
    assert lens[0] == 697 and lens[-1] == 69 and lens == sorted(lens, reverse=True)
    assert len(tfr.morlet(250.0, [100.0], 3.0)[0]) == 11
    assert len(tfr.morlet(1024.0, [2.8], 7.0)[0]) == 4075
    assert [len(W) for W in tfr.morlet(250.0, F_NB, F_NB / 2.0)] == [199] * 37
    assert len(tfr.morlet(250.0, 10.0)) == 1                       # a scalar frequency


def test_value_errors(tfr):
    x = np.zeros((2, 3, 800))
    call = tfr.tfr_array_morlet
    assert tfr.MAX_TAPS >= 4095 and tfr.MAX_FREQS >= 256
    with pytest.raises(ValueError, match="696"):                   # 4 Hz x 7 cycles: 697 taps
        call(np.zeros((1, 1, 696)), 250.0, [4.0])
    with pytest.raises(ValueError, match="longer than the signal"):
        tfr.cwt(np.zeros((1, 32)), [np.ones(33, dtype=complex)])
    with pytest.raises(ValueError, match="non-empty"):
        call(x, 250.0, [])
    with pytest.raises(ValueError, match="-3"):
        call(x, 250.0, [10.0, -3.0])
    with pytest.raises(ValueError, match="positive"):
        call(x, 250.0, [0.0, 10.0])
    with pytest.raises(ValueError, match="125"):
        call(x, 250.0, [10.0, 125.0])
    with pytest.raises(ValueError, match="Nyquist"):
        call(x, 250.0, [130.0])
    with pytest.raises(ValueError, match="n_cycles"):
        call(x, 250.0, [10.0, 20.0, 30.0], n_cycles=[3.0, 4.0])
    with pytest.raises(ValueError, match="n_cycles"):
        tfr.morlet(250.0, [10.0, 20.0], n_cycles=[3.0, 4.0, 5.0])
    for decim in (0, -2):
        with pytest.raises(ValueError, match=f"decim={decim}"):
            call(x, 250.0, [20.0], decim=decim)
    for output in ("avg_power", "itc", "avg_power_itc"):
        with pytest.raises(ValueError, match="n=0"):
            call(np.zeros((0, 3, 800)), 250.0, [20.0], output=output)
    with pytest.raises(ValueError, match="'amplitude'"):
        call(x, 250.0, [20.0], output="amplitude")
    with pytest.raises(ValueError, match="axes"):
        call(np.zeros((3, 800)), 250.0, [20.0])
    with pytest.raises(ValueError, match="even|odd"):
        tfr.cwt(np.zeros((1, 64)), [np.ones(4, dtype=complex)])


def test_not_implemented_errors(tfr):
    x = np.zeros((1, 1, 5000))
    call = tfr.tfr_array_morlet
    with pytest.raises(NotImplementedError, match="slice"):
        call(x, 250.0, [20.0], decim=slice(0, None, 2))
    assert 4096 <= len(tfr.morlet(1024.0, [2.7], 7.0)[0]) < 5000    # past the 4095 of the envelope, within T
    with pytest.raises(NotImplementedError, match="MAX_TAPS"):
        call(x, 1024.0, [2.7], n_cycles=7.0)
    with pytest.raises(NotImplementedError, match="MAX_FREQS"):
        call(x, 1024.0, np.linspace(100.0, 400.0, tfr.MAX_FREQS + 1), n_cycles=3.0)
    with pytest.raises(NotImplementedError, match="MAX_DECIM"):
        call(x, 250.0, [20.0], decim=tfr.MAX_DECIM + 1)
    with pytest.raises(NotImplementedError, match="mode"):
        tfr.cwt(np.zeros((1, 64)), [np.ones(5, dtype=complex)], mode="full")


def test_type_errors(tfr):
    call = tfr.tfr_array_morlet
    with pytest.raises(TypeError, match="GPU"):
        call(torch.zeros(2, 3, 800), 250.0, [20.0])                # a CPU tensor
    with pytest.raises(TypeError, match="GPU"):
        tfr.cwt(torch.zeros(2, 800), [np.ones(5, dtype=complex)])
    with pytest.raises(TypeError, match="floating"):
        call(np.zeros((2, 3, 800), dtype=np.int32), 250.0, [20.0])
    with pytest.raises(TypeError, match="floating"):
        call(np.zeros((2, 3, 800), dtype=np.complex128), 250.0, [20.0])
    with pytest.raises(TypeError, match="decim"):
        call(np.zeros((2, 3, 800)), 250.0, [20.0], decim=2.0)
    with pytest.raises(TypeError, match="floating"):
        call([[[1, 2, 3]]], 250.0, [20.0])                          # a nested list is taken as an array
    with pytest.raises(ValueError, match="axes"):
        call([[1.0, 2.0, 3.0]], 250.0, [20.0])


def test_wavelet_as_long_as_the_signal_is_accepted(tfr):
    """T = 697 passes every host check (what follows needs the GPU or fails for the lack of one); T = 696 does not."""
    n_taps = tuple(len(W) for W in tfr.morlet(250.0, [4.0], 7.0, zero_mean=True))
    assert n_taps == (697,)
    tfr._check_taps(n_taps, 697)
    with pytest.raises(ValueError, match="697 taps against 696"):
        tfr._check_taps(n_taps, 696)


@pytest.mark.parametrize("decim", [1, 2, 3, 7])
def test_out_len(tfr, decim):
    for T in (1, 6, 7, 8, 96, 795, 2500):
        assert tfr.out_len(T, decim) == len(range(0, T, decim)) == int(np.ceil(T / decim))
        if T >= 8:
            assert tfr_ref.cwt(np.zeros((1, T)), [np.ones(5, dtype=complex)], decim).shape == (1, 1, tfr.out_len(T, decim))


def test_reference_phase_mask_keeps_most_samples():
    """The phase comparison of test_tfr_gpu.py looks only where |z| exceeds 1e-3 of its row's maximum: in the
    reference alone that keeps well over the 90 % the GPU test asserts."""
    for name in ("A", "D"):
        shape, sfreq, freqs, n_cycles = tfr_ref.CASES[name]
        z = tfr_ref.tfr(tfr_ref.make_data(shape, sfreq), sfreq, freqs, n_cycles)["complex"]
        mag = np.abs(z)
        kept = (mag > 1e-3 * mag.max(-1, keepdims=True)).mean()
        print(f"case {name}: the mask keeps {kept:.1%}")
        assert kept > 0.95


def test_every_header_entry_is_declared():
    from isd_amd import _lib
    with open(os.path.join(ROOT, "include", "isd_hip.h")) as fh:
        names = set(re.findall(r"\b(isd_tfr_\w+)\s*\(", fh.read()))
    assert {"isd_tfr_plan_create", "isd_tfr_plan_destroy", "isd_tfr_plan_out_len", "isd_tfr_work_bytes",
            "isd_tfr_cwt_f32", "isd_tfr_cwt_f64"} <= names
    for name in names:
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["isd_tfr_plan_create"][1]) == 5
    assert len(_lib.SIGNATURES["isd_tfr_work_bytes"][1]) == 6
    assert len(_lib.SIGNATURES["isd_tfr_cwt_f32"][1]) == len(_lib.SIGNATURES["isd_tfr_cwt_f64"][1]) == 9


def test_import_does_not_load_the_library():
    code = ("import isd_amd, isd_amd.tfr, isd_amd._lib as L; "
            "assert isd_amd.tfr_array_morlet is isd_amd.tfr.tfr_array_morlet; "
            "assert 'tfr' in isd_amd.__all__ and 'tfr_array_morlet' in isd_amd.__all__; "
            "isd_amd.tfr.morlet(250, [10.0, 20.0]); assert L._lib is None; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
