"""What needs no GPU of isd_amd.analytic and isd_amd.connectivity.envelope_correlation: the NumPy restatement of
tests/envelope_ref.py against scipy and np.corrcoef, its degenerate cases, the argument errors, the ABI and the
import."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.signal as ss
import torch

from envelope_ref import CASES, make, ref_envcorr, ref_hilbert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1, 2, 64, 65, 795]


def lengths_of(T):
    """N of the hilbert tests: default, shorter, longer (where the shorter one is still a length)."""
    return [N for N in (None, T - 3, T + 29) if N is None or N >= 1]


@pytest.mark.parametrize("T", LENGTHS)
def test_restated_hilbert_is_scipy(T):
    x = make(2, 3, T, 7)
    for N in lengths_of(T):
        want = ss.hilbert(x, N, axis=-1)
        got = ref_hilbert(x, N)
        assert got.shape == want.shape == (2, 3, T if N is None else N)
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("case", ["a", "b", "c1"])
@pytest.mark.parametrize("log", [False, True])
def test_restated_plain_correlation_is_corrcoef(case, log):
    z = ss.hilbert(make(*CASES[case], 1), axis=-1)
    got = ref_envcorr(z, orthogonalize=False, log=log)
    for i in range(z.shape[0]):
        e = np.log(np.abs(z[i]) ** 2) if log else np.abs(z[i])
        assert np.abs(got[i] - np.atleast_2d(np.corrcoef(e))).max() <= 1e-14


def test_restated_pairwise_structure_and_span():
    for case in ("a", "b", "c"):
        z = ss.hilbert(make(*CASES[case], 1), axis=-1)
        for log in (False, True):
            got = ref_envcorr(z, log=log)
            assert np.isfinite(got).all() and np.array_equal(got, got.transpose(0, 2, 1))
            assert (np.diagonal(got, axis1=1, axis2=2) == 0).all()
            off = got[:, ~np.eye(z.shape[1], dtype=bool)]
            assert off.min() >= 0 and 0.05 < off.max() < 0.6
            signed = ref_envcorr(z, log=log, absolute=False)
            assert (np.abs(signed) <= got + 1e-15).all() and signed.min() < 0


def test_restated_degenerate_cases():
    z = ss.hilbert(make(*CASES["t1"], 2), axis=-1)                      # T = 1 (its analytic signal is real)
    zc = z + 1j * make(*CASES["t1"], 6)                                 # T = 1, complex: log o is finite
    for orth in ("pairwise", False):
        assert not ref_envcorr(z, orth).any()
        for log in (False, True):
            assert not ref_envcorr(zc, orth, log).any()
    z = make(*CASES["t2"], 3).astype(np.complex128)                     # real-valued z, T = 2
    assert not ref_envcorr(z).any() and not ref_envcorr(z, absolute=False).any()
    z = ss.hilbert(make(*CASES["c1"], 4), axis=-1)                      # C = 1
    assert ref_envcorr(z).shape == (2, 1, 1) and not ref_envcorr(z).any()
    assert np.abs(ref_envcorr(z, orthogonalize=False) - 1).max() <= 1e-15
    z = ss.hilbert(make(*CASES["a"], 5), axis=-1)                       # a dead channel
    z[:, 2] = 0
    for orth in ("pairwise", False):
        got = ref_envcorr(z, orth)
        assert np.isfinite(got).all() and not got[:, 2].any() and not got[:, :, 2].any()
        live = np.delete(np.delete(got, 2, 1), 2, 2)
        assert np.abs(live - ref_envcorr(np.delete(z, 2, 1), orth)).max() <= 1e-14
    with_nan = ref_envcorr(z, log=True)                                  # log: NaN where the zero enters, only there
    others = [0, 1, 3, 4]
    assert np.isnan(with_nan[:, 2, others]).all() and np.isnan(with_nan[:, others, 2]).all()
    assert np.isfinite(np.delete(np.delete(with_nan, 2, 1), 2, 2)).all()


def test_argument_errors_need_no_gpu():
    from isd_amd import analytic, connectivity as con
    x = np.zeros((2, 129, 16))
    with pytest.raises(NotImplementedError, match="129"):
        con.envelope_correlation(x)
    with pytest.raises(NotImplementedError, match="129"):
        con.envelope_correlation(x.astype(np.complex128), orthogonalize=False)
    x = np.zeros((2, 4, 16))
    for bad in ("x", True, None, "Pairwise"):
        with pytest.raises(ValueError, match="orthogonalize"):
            con.envelope_correlation(x, orthogonalize=bad)
    for fn in (con.envelope_correlation, analytic.hilbert, analytic.envelope):
        with pytest.raises(TypeError):
            fn(np.zeros((2, 4, 16), dtype=np.int32))
        with pytest.raises(TypeError):
            fn(torch.zeros(2, 4, 16))                                    # a CPU tensor
    with pytest.raises(ValueError):
        con.envelope_correlation(np.zeros(16))
    with pytest.raises(ValueError):
        con.envelope_correlation(np.zeros((1, 2, 4, 16)))
    with pytest.raises(ValueError):
        con.envelope_correlation(np.zeros((2, 4, 0)))
    for N in (0, -1, 2.5):
        with pytest.raises(ValueError):
            analytic.hilbert(np.zeros(8), N)
    assert con.MAX_CHANNELS == 128 and "envelope_correlation" not in con.METHODS


def test_abi_names_and_header():
    from isd_amd import _lib
    header = open(os.path.join(ROOT, "include", "isd_hip.h")).read()
    for name, n_args in (("isd_envcorr_work_bytes", 4), ("isd_envcorr_f32", 8), ("isd_envcorr_f64", 8)):
        assert len(_lib.SIGNATURES[name][1]) == n_args
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert _lib.SIGNATURES["isd_envcorr_work_bytes"][0] is _lib._i64


def test_import_does_not_load_the_library():
    code = ("import isd_amd, isd_amd.analytic, isd_amd._lib as L; "
            "assert isd_amd.hilbert is isd_amd.analytic.hilbert and isd_amd.envelope is isd_amd.analytic.envelope; "
            "assert {'analytic', 'hilbert', 'envelope'} <= set(isd_amd.__all__); "
            "assert callable(isd_amd.connectivity.envelope_correlation); "
            "assert L._lib is None; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
