"""What needs no GPU of isd_amd.pac: the NumPy restatement of tests/pac_ref.py against closed forms, the binning
rule, draw_shifts, the argument errors (all raised before any GPU use), the ABI and the import."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pac_ref import CASES, METHODS, make_case, ref_bins, ref_block, ref_pac, ref_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------- the restatement, closed forms
def test_constant_amplitude():
    rng = np.random.default_rng(1)
    pha = rng.uniform(-np.pi, np.pi, (2, 200))
    amp = np.full((1, 200), 2.5)
    mvl, mi, hr = ref_pac(pha, amp, [0, 7, 150], 18)
    assert np.abs(mi).max() <= 1e-15 and np.abs(hr).max() <= 1e-15
    want = 2.5 * np.abs(np.exp(1j * pha).mean(-1))
    assert np.abs(mvl - want[None, :, None]).max() <= 1e-15


def test_amplitude_in_one_bin_only():
    B, T = 18, 180
    pha = (-np.pi + (np.arange(T) % B + 0.5) * 2 * np.pi / B)[None]
    amp = np.where(ref_bins(pha[0], B) == 5, 3.0, 0.0)[None]
    mvl, mi, hr = ref_pac(pha, amp, [0], B)
    assert abs(mi[0, 0, 0] - 1.0) <= 1e-15 and hr[0, 0, 0] == 1.0


def test_one_sample():
    mvl, mi, hr = ref_pac(np.array([[0.3]]), np.array([[1.7]]), [0], 18)
    assert mi[0, 0, 0] == 1.0 and hr[0, 0, 0] == 1.0 and abs(mvl[0, 0, 0] - 1.7) <= 1e-15


@pytest.mark.parametrize("B,k,m", [(18, 4, 0.5), (3, 3, 0.9), (64, 2, 0.25)])     # B >= 3: mean cos^2 = 1 / 2
def test_cosine_modulation_at_the_bin_centres(B, k, m):
    centres = -np.pi + (np.arange(B) + 0.5) * 2 * np.pi / B
    pha = np.tile(centres, k)[None]
    amp = 1.0 + m * np.cos(pha)
    assert np.array_equal(ref_bins(pha[0], B), np.tile(np.arange(B), k))
    mvl, mi, hr = ref_pac(pha, amp, [0], B)
    assert abs(mvl[0, 0, 0] - m / 2) <= 1e-15
    Pj = (1.0 + m * np.cos(centres)) / B
    assert abs(mi[0, 0, 0] - (1.0 + (Pj * np.log(Pj)).sum() / np.log(B))) <= 1e-15
    assert abs(hr[0, 0, 0] - (Pj.max() - Pj.min()) / Pj.max()) <= 1e-15


def test_a_shift_is_a_roll_of_the_amplitude():
    pha, amp, shifts, B = make_case(1)
    for s in (1, 17, 36):
        got = ref_pac(pha[0], amp[0], [0, s], B)
        want = ref_pac(pha[0], np.roll(amp[0], -s, axis=-1), [0], B)
        for g, w in zip(got, want):
            assert np.abs(g[..., 1] - w[..., 0]).max() <= 1e-15         # (a matrix product of another shape)


def test_stats_and_block_layout():
    pha, amp, shifts, B = make_case(1)
    block, surr = ref_block(pha, amp, shifts, B)
    assert block.shape == (3, 3, 2, 3, 4) and surr.shape == (3, 3, 2, 3, 5)
    v = ref_pac(pha[2], amp[2], shifts, B)[1]                            # 'mi' of row 2
    assert np.array_equal(block[2, :, :, 1, 0], v[..., 0]) and np.array_equal(surr[2, :, :, 1], v[..., 1:])
    mean, std, n_ge = ref_stats(v)
    assert np.array_equal(block[2, :, :, 1, 1], mean) and np.array_equal(block[2, :, :, 1, 3], n_ge)
    assert np.abs(std - np.sqrt(((v[..., 1:] - mean[..., None]) ** 2).mean(-1))).max() <= 1e-16
    mean, std, n_ge = ref_stats(v[..., :1])
    assert np.isnan(mean).all() and np.isnan(std).all() and not n_ge.any()
    assert sorted(CASES) == list(range(1, 11)) and METHODS == ("mvl", "mi", "hr")


# --------------------------------------------------------------------------------------------------------- binning
def test_binning_rule():
    for B in (2, 18, 64):
        phi = np.array([-np.pi, np.float64(np.float32(np.pi)), np.pi, 0.0])
        b = ref_bins(phi, B)
        assert b[0] == 0 and b[1] == B - 1 and b[2] == B - 1
        assert b[3] == min(B - 1, max(0, math.floor((0.0 + math.pi) * (B / (2.0 * math.pi)))))
        assert ref_bins(np.array([np.pi], dtype=np.float32), B)[0] == B - 1
    pha = make_case(7)[0]
    assert set(np.unique(ref_bins(pha, 18))) <= set(range(9, 14))         # [0, pi / 2]: the other bins are empty


# ----------------------------------------------------------------------------------------------------- draw_shifts
def test_draw_shifts():
    from isd_amd import pac
    a, b = pac.draw_shifts(795, 200, 3), pac.draw_shifts(795, 200, 3)
    assert a.dtype == np.int32 and a.shape == (201,) and np.array_equal(a, b)
    assert not np.array_equal(a, pac.draw_shifts(795, 200, 4))
    assert a[0] == 0 and a[1:].min() >= 1 and a[1:].max() <= 794
    c = pac.draw_shifts(100, 500, 0, min_shift=40)
    assert c[0] == 0 and c[1:].min() >= 40 and c[1:].max() <= 60 and set(c[1:]) == set(range(40, 61))
    assert np.array_equal(pac.draw_shifts(2, 3, 0), [0, 1, 1, 1])
    assert np.array_equal(pac.draw_shifts(50, 0), [0])
    for T, ms in ((1, 1), (79, 40), (0, 1)):
        with pytest.raises(ValueError):
            pac.draw_shifts(T, 4, 0, min_shift=ms)


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_need_no_gpu(monkeypatch):
    import isd_amd
    from isd_amd import _lib, pac

    def no_gpu(*a, **k):
        raise AssertionError("the GPU or the library was used before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_gpu)
    monkeypatch.setattr(_lib, "to_device", no_gpu)

    x = np.zeros((2, 3, 400))
    ok = dict(sfreq=250.0, f_pha=[(4, 8)], f_amp=[(30, 50)])
    call = isd_amd.phase_amplitude_coupling
    with pytest.raises(ValueError, match="unknown method"):
        call(x, **ok, method="tort")
    with pytest.raises(ValueError, match="unknown method"):
        call(x, **ok, method=["mi", "tort"])
    for name in ("ndpac", "plv", "gc"):
        with pytest.raises(NotImplementedError, match=name):
            call(x, **ok, method=name)
        with pytest.raises(NotImplementedError, match=name):
            call(x, **ok, method=["mi", name])
    with pytest.raises(NotImplementedError, match="swap_trials"):
        call(x, **ok, surrogate="swap_trials")
    with pytest.raises(ValueError, match="n_bins"):
        call(x, **ok, n_bins=1)
    with pytest.raises(NotImplementedError, match="64"):
        call(x, **ok, n_bins=65)
    with pytest.raises(ValueError, match="f_pha"):
        call(x, 250.0, [], [(30, 50)])
    with pytest.raises(ValueError, match="f_amp"):
        call(x, 250.0, [(4, 8)], [])
    with pytest.raises(ValueError, match="lo < hi"):
        call(x, 250.0, [(8, 8)], [(30, 50)])
    with pytest.raises(ValueError, match="lo < hi"):
        call(x, 250.0, [(4, 8)], [(50, 30)])
    with pytest.raises(ValueError, match="edges"):
        call(x, **ok, edges=200)
    with pytest.raises(ValueError, match="edges"):
        call(x, **ok, edges=-1)
    for norm in ("zscore", "subtract", "divide", "subtract_divide"):
        with pytest.raises(ValueError, match="needs surrogates"):
            call(x, **ok, normalize=norm)
    with pytest.raises(ValueError, match="normalize"):
        call(x, **ok, normalize="z", n_surrogates=4)
    with pytest.raises(NotImplementedError, match="4096"):
        call(np.zeros((1, 2, 4097)), **ok)
    with pytest.raises(NotImplementedError, match="4096"):
        call(np.zeros((1, 2, 4099)), **ok, edges=1)
    with pytest.raises(NotImplementedError, match="4095"):
        call(x, **ok, n_surrogates=4096)
    with pytest.raises(TypeError):
        call(np.zeros((2, 3, 400), dtype=np.int32), **ok)
    with pytest.raises(TypeError):
        call(torch.zeros(2, 3, 400), **ok)                               # a CPU tensor
    with pytest.raises(ValueError):
        call(np.zeros(400), **ok)
    with pytest.raises(ValueError, match="shifts"):
        call(x, **ok, shifts=[1, 2, 3])                                  # no leading 0
    with pytest.raises(ValueError, match="shifts"):
        call(x, **ok, shifts=[0, 400])                                   # >= T'
    with pytest.raises(ValueError, match="n_fft"):
        call(x, **ok, n_fft=399)
    assert pac.MAX_T == 4096 and pac.MAX_BINS == 64 and pac.MAX_SURROGATES == 4095 and pac.METHODS == METHODS
    for bad in (torch.zeros(2, 3, 8), np.zeros((2, 3, 8))):              # pac_launch takes CUDA tensors only
        with pytest.raises(TypeError):
            pac.pac_launch(bad, bad, [0])


# --------------------------------------------------------------------------------------------------------------- ABI
def test_abi_names_and_header():
    from isd_amd import _lib
    header = open(os.path.join(ROOT, "include", "isd_hip.h")).read()
    for name, n_args in (("isd_pac_work_bytes", 5), ("isd_pac_f32", 14), ("isd_pac_f64", 14)):
        assert len(_lib.SIGNATURES[name][1]) == n_args
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args, name
    assert _lib.SIGNATURES["isd_pac_work_bytes"][0] is _lib._i64


def test_library_refuses_what_is_outside_the_envelope():
    import __graft_entry__
    __graft_entry__.build()
    from isd_amd import _lib
    L = _lib.lib()
    assert L.isd_pac_work_bytes(4, 2, 3, 795, 0) > 0 and L.isd_pac_work_bytes(0, 1, 1, 1, 1) > 0
    assert L.isd_pac_work_bytes(4, 2, 3, 4097, 0) == _lib.ISD_ERR_UNSUPPORTED and b"4097" in L.isd_last_error()
    assert L.isd_pac_work_bytes(4, 0, 3, 16, 0) == _lib.ISD_ERR_INVALID

    def call(rows=1, P=1, A=1, T=16, S=0, B=18):
        rc = L.isd_pac_f32(None, None, None, None, None, rows, P, A, T, S, B, B / (2 * np.pi), None, None)
        return rc, L.isd_last_error()

    assert call(rows=0)[0] == _lib.ISD_OK                                # nothing to do, nothing touched
    for kw, frag in ((dict(T=4097), b"4096"), (dict(B=1), b"n_bins=1"), (dict(B=65), b"64"), (dict(S=4096), b"4095"),
                     (dict(rows=1 << 20, P=1 << 6, A=1 << 5), b"2^31")):
        rc, msg = call(**kw)
        assert rc == _lib.ISD_ERR_UNSUPPORTED and frag in msg, (kw, msg)
    for kw in (dict(T=0), dict(P=0), dict(S=-1)):
        assert call(**kw)[0] == _lib.ISD_ERR_INVALID
    rc, msg = call()
    assert rc == _lib.ISD_ERR_INVALID and b"null" in msg


def test_import_does_not_load_the_library():
    code = ("import isd_amd, isd_amd.pac, isd_amd._lib as L; "
            "assert isd_amd.phase_amplitude_coupling is isd_amd.pac.phase_amplitude_coupling; "
            "assert {'pac', 'phase_amplitude_coupling'} <= set(isd_amd.__all__); "
            "assert callable(isd_amd.pac.pac_launch) and callable(isd_amd.pac.draw_shifts); "
            "assert L._lib is None; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
