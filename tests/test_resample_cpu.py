"""isd_amd.resampling without a GPU and without loading the library: the design against scipy.signal.firwin, out_len
against scipy, the NumPy restatement of tests/resample_ref.py against scipy.signal.resample_poly itself (scipy is the
reference the GPU tests use; the restatement is the formula the kernel implements), every argument error, and the C
ABI's declarations.  The phase tables are built inside the library, so there is no table test here.

scipy dies with a floating point exception for a one-sample row with a non-constant upfirdn mode: no case here hands
it one."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import signal

import resample_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rs():
    from isd_amd import resampling
    return resampling


@pytest.mark.parametrize("up,down,red", [(1, 4, (1, 4)), (4, 1, (4, 1)), (3, 2, (3, 2)), (125, 512, (125, 512)),
                                         (160, 147, (160, 147)), (4, 16, (1, 4)), (250, 1024, (125, 512))])
def test_design_is_firwin_times_up(rs, up, down, red):
    d = rs.resample_design(up, down)
    assert (d.up, d.down) == red
    m = max(red)
    ref = signal.firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0)) * red[0]
    assert d.half_len == 10 * m and d.taps.dtype == np.float64 and d.taps.shape == ref.shape
    assert np.max(np.abs(d.taps - ref)) <= 2e-16 * np.max(np.abs(ref))


def test_design_window_name_and_explicit_taps(rs):
    d = rs.resample_design(3, 2, window="hamming")
    ref = signal.firwin(61, 1.0 / 3, window="hamming") * 3
    assert np.max(np.abs(d.taps - ref)) <= 2e-16 * np.max(np.abs(ref))
    for n, taps in resample_ref.TAPS.items():                      # 1, 2, 31, 32 taps: even lengths are allowed
        for window in (taps, list(taps)):
            d = rs.resample_design(6, 4, window=window)
            assert (d.up, d.down, d.half_len) == (3, 2, (n - 1) // 2)
            assert np.max(np.abs(d.taps - 3 * taps)) <= 2e-16 * np.max(np.abs(3 * taps))
    taps = resample_ref.TAPS[31].copy()
    d = rs.resample_design(1, 2, window=taps)
    taps[:] = 0                                                    # the design does not alias the caller's array
    assert np.any(d.taps != 0)
    d = rs.resample_design(5, 5)                                   # scipy copies: the identity
    assert (d.up, d.down, d.half_len) == (1, 1, 0) and d.taps.tolist() == [1.0]


@pytest.mark.parametrize("up,down", resample_ref.RATIOS + [(250, 1024), (1024, 1), (1, 1024)])
def test_out_len(rs, up, down):
    for T in (1, 2, 3, 5, 37, 64, 600, 795):
        assert rs.out_len(T, up, down) == len(signal.resample_poly(np.zeros(T), up, down)), (up, down, T)


SHAPES = [(1, 2, 795), (1, 4, 37), (2, 1, 5), (7, 1, 2), (3, 2, 37), (2, 3, 795), (125, 512, 600), (160, 147, 100),
          (4, 16, 64), (1, 4, 3), (7, 1, 37), (2, 3, 2)]


@pytest.mark.parametrize("up,down,T", SHAPES)
def test_restatement_against_scipy(up, down, T):
    x = resample_ref.make_rows(3, T)
    worst = 0.0
    for padtype in resample_ref.PADTYPES:
        ref = signal.resample_poly(x, up, down, axis=-1, padtype=padtype)
        worst = max(worst, resample_ref.rel_err(resample_ref.resample_poly(x, up, down, padtype=padtype), ref))
    ref = signal.resample_poly(x, up, down, axis=-1, cval=2.5)
    worst = max(worst, resample_ref.rel_err(resample_ref.resample_poly(x, up, down, cval=2.5), ref))
    for taps in resample_ref.TAPS.values():
        ref = signal.resample_poly(x, up, down, axis=-1, window=taps, padtype="edge")
        worst = max(worst, resample_ref.rel_err(resample_ref.resample_poly(x, up, down, window=taps, padtype="edge"),
                                                ref))
    print(f"{up}/{down} T={T}: restatement against scipy {worst:.2e}")
    assert worst <= 1e-13


def test_restatement_one_sample_rows():
    x = resample_ref.make_rows(3, 1)                               # 'constant' and the statistics only: see above
    for up, down in ((1, 2), (7, 1), (3, 2)):
        for padtype in ("constant", "mean", "median", "minimum", "maximum"):
            ref = signal.resample_poly(x, up, down, axis=-1, padtype=padtype)
            assert resample_ref.rel_err(resample_ref.resample_poly(x, up, down, padtype=padtype), ref) <= 1e-13


def test_value_errors(rs):
    x = np.zeros((2, 8))
    for up, down in ((0, 1), (1, 0), (-2, 1), (1.5, 1), (1, 2.5), ("a", 1)):
        with pytest.raises(ValueError):
            rs.resample_poly(x, up, down)
        with pytest.raises(ValueError):
            rs.resample_design(up, down)
    with pytest.raises(ValueError):
        rs.out_len(8, 0, 1)
    for padtype in ("edge", "reflect", "mean", "line"):
        with pytest.raises(ValueError, match="cval"):
            rs.resample_poly(x, 1, 2, padtype=padtype, cval=1.0)
    for padtype in ("nearest", "zeros", None, 3):
        with pytest.raises(ValueError, match="padtype"):
            rs.resample_poly(x, 1, 2, padtype=padtype)
    for padtype in ("reflect", "line"):
        with pytest.raises(ValueError, match="two samples"):
            rs.resample_poly(np.zeros((2, 1)), 1, 2, padtype=padtype)
    with pytest.raises(ValueError):
        rs.resample_poly(np.zeros((2, 0)), 1, 2)
    with pytest.raises(ValueError):
        rs.resample_poly(np.float64(1.0), 1, 2)
    with pytest.raises(ValueError, match="axis"):
        rs.resample_poly(x, 1, 2, axis=2)
    for window in (np.zeros((2, 3)), np.zeros(0), [1.0, np.nan]):
        with pytest.raises(ValueError, match="window"):
            rs.resample_design(1, 2, window=window)
    for up, down in ((0, 1), (1, -1), (float("inf"), 1)):
        with pytest.raises(ValueError):
            rs.resample(x, up=up, down=down)


def test_not_implemented_errors(rs):
    x = np.zeros((2, 8))
    for padtype in ("wrap", "smooth", "antireflect", "antisymmetric"):
        with pytest.raises(NotImplementedError, match=padtype):
            rs.resample_poly(x, 1, 2, padtype=padtype)
    with pytest.raises(NotImplementedError, match="1024"):
        rs.resample_poly(x, 1025, 1)
    with pytest.raises(NotImplementedError, match="1024"):
        rs.resample_poly(x, 1, 1025, window=np.ones(3))
    with pytest.raises(NotImplementedError, match="20481"):
        rs.resample_poly(x, 1, 2, window=np.ones(20482))
    with pytest.raises(NotImplementedError, match="fft"):
        rs.resample(x, up=1, down=2, method="fft")
    with pytest.raises(NotImplementedError, match="fft"):
        rs.resample(x, 1, 2, npad=100, method="fft")
    with pytest.raises(NotImplementedError, match="wrap"):
        rs.resample(x, 1, 2, pad="wrap")


def test_type_errors_and_no_cpu_fallback(rs):
    with pytest.raises(TypeError):
        rs.resample_poly(torch.zeros(2, 8), 1, 2)                  # a CPU tensor
    with pytest.raises(TypeError):
        rs.resample_poly(np.zeros((2, 8), dtype=np.int32), 1, 2)
    with pytest.raises(TypeError):
        rs.resample_poly(np.zeros((2, 8), dtype=np.complex128), 1, 2)
    with pytest.raises(TypeError):
        rs.resample(torch.zeros(2, 8), up=1, down=2)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            rs.resample_poly(np.zeros((2, 8)), 1, 2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            rs.resample(np.zeros((2, 8)), up=250, down=1024)


def test_every_header_entry_is_declared():
    from isd_amd import _lib
    with open(os.path.join(ROOT, "include", "isd_hip.h")) as fh:
        names = set(re.findall(r"\b(isd_resample_\w+)\s*\(", fh.read()))
    assert names == {"isd_resample_plan_create", "isd_resample_plan_destroy", "isd_resample_out_len",
                     "isd_resample_poly_f32", "isd_resample_poly_f64"}
    for name in names:
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["isd_resample_plan_create"][1]) == 6
    assert len(_lib.SIGNATURES["isd_resample_plan_destroy"][1]) == 1
    assert len(_lib.SIGNATURES["isd_resample_out_len"][1]) == 2
    assert len(_lib.SIGNATURES["isd_resample_poly_f32"][1]) == len(_lib.SIGNATURES["isd_resample_poly_f64"][1]) == 9


def test_library_refuses_outside_the_envelope_without_a_device():
    """isd_resample_plan_create checks its arguments before it looks for a device."""
    import ctypes as C
    import __graft_entry__
    __graft_entry__.build()
    from isd_amd import _lib
    L = _lib.lib()
    taps = _lib.double_array([1.0, 2.0, 1.0])
    for args, code in (((1025, 1, 3, taps, 1), _lib.ISD_ERR_UNSUPPORTED), ((1, 1025, 3, taps, 1), _lib.ISD_ERR_UNSUPPORTED),
                       ((1, 2, 20482, _lib.double_array(np.ones(20482)), 0), _lib.ISD_ERR_UNSUPPORTED),
                       ((2, 4, 3, taps, 1), _lib.ISD_ERR_INVALID), ((0, 1, 3, taps, 1), _lib.ISD_ERR_INVALID),
                       ((1, 2, 3, taps, 3), _lib.ISD_ERR_INVALID), ((1, 2, 0, taps, 0), _lib.ISD_ERR_INVALID)):
        h = C.c_void_p()
        assert L.isd_resample_plan_create(C.byref(h), *args) == code, args
        assert not h.value
    assert L.isd_resample_plan_destroy(None) == _lib.ISD_OK
    assert L.isd_resample_out_len(None, 8) < 0


def test_import_does_not_load_the_library():
    code = ("import isd_amd, isd_amd.resampling, isd_amd._lib as L; "
            "assert isd_amd.resample_poly is isd_amd.resampling.resample_poly; "
            "assert isd_amd.resample is isd_amd.resampling.resample and isd_amd.resample_mod is isd_amd.resampling; "
            "assert {'resample_poly', 'resample', 'resample_mod'} <= set(isd_amd.__all__); "
            "isd_amd.resampling.resample_design(1, 4); assert isd_amd.resampling.out_len(4096, 250, 1024) == 1000; "
            "assert L._lib is None; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
