"""isd_amd.tfr_array_morlet / tfr.cwt on the GPU against the NumPy complex128 restatement of tests/tfr_ref.py.

Data: standard_normal + 2 sin(2 pi 10 t) + a per-trial offset cycling through 0, 50, -200.  For float32 the reference
sees the float32-rounded input widened to float64.  Cases (tfr_ref.CASES): A T below one tile, 11 .. 59 taps; B 17
frequencies of equal length; C taps == T; D 697 and 69 taps in one call; E the 4075-tap envelope on T beyond one time
tile; F several time tiles and five trials.  The kernel's time tile is at most 512 outputs, so the issue asks for no
case beyond these; G (32 channels x 3000 samples, 17 frequencies in three groups) is added because the averaged kernels
shorten their tile to one chunk of 128 outputs when there are few (channel, tile) pairs, as in A - F: on G they keep
512 outputs (four chunks, one group per workgroup), and B puts three groups into one workgroup.

Bounds: the largest absolute error over the largest |reference|, taken over the whole call and separately per
(trial, channel) row (per channel for the averaged outputs), below TOL64 = 1e-12 / TOL32 = 1e-5 (test_fir_gpu.py,
test_csp_gpu.py, test_psd_gpu.py).  A complex64 NumPy restatement of the same sums deviates from fp64 by 1.8e-7 ..
5.6e-7 (complex) and 2.1e-7 .. 1.1e-6 (power) on these cases, so 1e-5 leaves about 10x over fp32 arithmetic itself.
'phase' is compared as |exp(i got) - exp(i ref)| where |ref z| exceeds 1e-3 of its (trial, channel, frequency) row's
maximum, against the same TOL64 / TOL32; the mask keeps over 95 % in the reference alone (test_tfr_cpu.py) and the test
asserts 90 %.  An error e of z relative to the row's maximum turns the phase of a sample at the mask's floor by 1e3 e,
and the same holds for 'itc', a mean of z / |z|: for float32 input the library therefore takes the product behind
both in fp64 over the widened samples.  In fp64 both sit just below the bound, where the restatement's own rounding is
of that size.

Observed on an MI355X (worst of whole-call and per-row error over the cases; each test prints its own figures):
  complex        fp64 5.1e-15 (E)   fp32 2.5e-6 (E, 4075 taps)     decim 2 / 3 / 7: 1.8e-15 / 9.6e-7 (F)
  power          fp64 7.3e-15 (E)   fp32 3.6e-6 (E)                decim: 3.1e-15 / 1.9e-6 (F)
  phase          fp64 9.6e-13 (D)   fp32 1.2e-7 (every case: the rounding of the angle itself); the mask keeps
                 99.6 - 100 % of the samples
  avg_power      fp64 3.3e-15 (D, n = 1)   fp32 1.9e-6 (F, n = 1);  B and G (three groups): 9.6e-16 / 1.9e-7
  itc            fp64 9.9e-13 (D)   fp32 3.0e-8 (B);  n = 1: |itc - 1| <= 3.3e-16 / 0
  cwt, asymmetric taps of 1, 5 and 33:  fp64 5.1e-16   fp32 2.0e-7
  avg_power of (16, 3, 300) fp32: peak memory rises by 61 952 bytes for a result of 61 200
"""
import ctypes as C

import numpy as np
import pytest
import torch

import tfr_ref
from tfr_ref import CASES

pytestmark = pytest.mark.gpu

TOL64, TOL32 = 1e-12, 1e-5
DTYPES = [(torch.float64, TOL64), (torch.float32, TOL32)]
AVERAGED = ("avg_power", "itc", "avg_power_itc")
_REFS = {}


@pytest.fixture(scope="module")
def isd():
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd


def case_data(case, dtype, n=None):
    """(float64 ndarray the reference sees, CUDA tensor of `dtype`); n keeps the first n trials."""
    shape, sfreq = CASES[case][:2]
    key = ("x", case, dtype)
    if key not in _REFS:
        x = tfr_ref.make_data(shape, sfreq)
        if dtype == torch.float32:
            x = x.astype(np.float32).astype(np.float64)
        x.setflags(write=False)
        _REFS[key] = x
    x = _REFS[key] if n is None else _REFS[key][:n]
    return x, torch.tensor(x, dtype=dtype).cuda()


def reference(case, dtype, decim=1, n=None):
    """The six outputs of the restatement, computed once per (case, dtype, decim, n) and left unchanged."""
    key = ("ref", case, dtype, decim, n)
    if key not in _REFS:
        x, _ = case_data(case, dtype, n)
        _, sfreq, freqs, n_cycles = CASES[case]
        ref = tfr_ref.tfr(x, sfreq, freqs, n_cycles, decim=decim)
        for v in ref.values():
            v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def call(isd, x, case, **kw):
    _, sfreq, freqs, n_cycles = CASES[case]
    return isd.tfr_array_morlet(x, sfreq, freqs, n_cycles, **kw)


def errors(got, ref, lead):
    """(error over the call, worst error of a row): rows are the first `lead` axes."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    d = np.abs(got.astype(ref.dtype) - ref).reshape((-1,) + ref.shape[lead:])
    r = np.abs(ref).reshape(d.shape)
    ax = tuple(range(1, d.ndim))
    return float(d.max() / r.max()), float((d.max(ax) / r.max(ax)).max())


def check(got, ref, lead, tol, what):
    assert tuple(got.shape) == ref.shape, (what, tuple(got.shape), ref.shape)
    whole, row = errors(got, ref, lead)
    print(f"{what}: max|err|/max|ref| = {whole:.2e} over the call, {row:.2e} worst row")
    assert whole < tol and row < tol, what


# ------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("case", sorted(CASES))
def test_complex_and_power_match_the_restatement(isd, case):
    for dtype, tol in DTYPES:
        _, xd = case_data(case, dtype)
        ref = reference(case, dtype)
        z = call(isd, xd, case)
        assert z.is_cuda and z.dtype == (torch.complex128 if dtype == torch.float64 else torch.complex64)
        check(z, ref["complex"], 2, tol, f"case {case} {str(dtype)[6:]} complex")
        p = call(isd, xd, case, output="power")
        assert p.is_cuda and p.dtype == dtype
        check(p, ref["power"], 2, tol, f"case {case} {str(dtype)[6:]} power")


@pytest.mark.parametrize("case", sorted(CASES))
def test_phase_matches_where_the_magnitude_is_not_negligible(isd, case):
    for dtype, tol in DTYPES:
        _, xd = case_data(case, dtype)
        ref = reference(case, dtype)
        got = call(isd, xd, case, output="phase")
        assert got.dtype == dtype and tuple(got.shape) == ref["phase"].shape
        mag = np.abs(ref["complex"])
        mask = mag > 1e-3 * mag.max(-1, keepdims=True)
        err = float(np.abs(np.exp(1j * got.cpu().numpy().astype(np.float64)) - np.exp(1j * ref["phase"]))[mask].max())
        print(f"case {case} {str(dtype)[6:]} phase: {err:.2e} over {mask.mean():.1%} of the samples")
        assert mask.mean() >= 0.9
        assert err < tol


@pytest.mark.parametrize("decim", [2, 3, 7])
@pytest.mark.parametrize("case", ["A", "F"])
def test_decimation(isd, case, decim):
    T = CASES[case][0][-1]
    for dtype, tol in DTYPES:
        _, xd = case_data(case, dtype)
        full, ref = reference(case, dtype), reference(case, dtype, decim)
        assert ref["complex"].shape[-1] == -(-T // decim)
        assert np.array_equal(ref["complex"], full["complex"][..., ::decim])
        for output, lead in (("complex", 2), ("power", 2), ("avg_power", 1)):
            got = call(isd, xd, case, decim=decim, output=output)
            check(got, ref[output], lead, tol, f"case {case} {str(dtype)[6:]} decim={decim} {output}")


@pytest.mark.parametrize("case", ["A", "B", "D", "F", "G"])
def test_averaged_outputs(isd, case):
    for dtype, tol in DTYPES:
        _, xd = case_data(case, dtype)
        ref = reference(case, dtype)
        got = {o: call(isd, xd, case, output=o) for o in AVERAGED}
        assert got["avg_power"].dtype == got["itc"].dtype == dtype
        assert got["avg_power_itc"].dtype == (torch.complex128 if dtype == torch.float64 else torch.complex64)
        for o in ("avg_power", "itc"):
            check(got[o], ref[o], 1, tol, f"case {case} {str(dtype)[6:]} {o}")
        assert float(got["itc"].max()) <= 1.0 + tol
        assert torch.equal(got["avg_power_itc"].real, got["avg_power"])           # bit for bit
        assert torch.equal(got["avg_power_itc"].imag, got["itc"])


@pytest.mark.parametrize("case", ["A", "D", "F"])
def test_one_trial_averages(isd, case):
    for dtype, tol in DTYPES:
        _, xd = case_data(case, dtype, n=1)
        ref = reference(case, dtype, n=1)
        power = call(isd, xd, case, output="power")
        avg, itc = call(isd, xd, case, output="avg_power"), call(isd, xd, case, output="itc")
        check(avg, ref["avg_power"], 1, tol, f"case {case} {str(dtype)[6:]} n=1 avg_power")
        assert torch.equal(avg, power[0])                           # the mean of one trial is that trial
        live = torch.abs(call(isd, xd, case)[0]) > 0
        assert live.float().mean() > 0.99
        dev = float((itc[live] - 1.0).abs().max())
        print(f"case {case} {str(dtype)[6:]} n=1: |itc - 1| <= {dev:.2e}")
        assert dev < tol and bool((itc[~live] == 0).all())


def test_convolution_direction(isd):
    """Asymmetric complex taps of lengths 1, 5 and 33: the conjugate-symmetric Morlet taps cannot tell w[k] from
    w[-k]."""
    rng = np.random.default_rng(11)
    Ws = [rng.standard_normal(L) + 1j * rng.standard_normal(L) for L in (1, 5, 33)]
    x = rng.standard_normal((3, 200))
    ref = np.stack([np.stack([np.convolve(r, W, "same") for W in Ws]) for r in x])
    for decim in (1, 3):
        got = isd.tfr.cwt(x, Ws, decim=decim)
        assert isinstance(got, np.ndarray) and got.dtype == np.complex128
        check(got, ref[..., ::decim], 1, TOL64, f"cwt decim={decim} float64")
        got32 = isd.tfr.cwt(torch.tensor(x, dtype=torch.float32).cuda(), Ws, decim=decim)
        assert got32.is_cuda and got32.dtype == torch.complex64
        ref32 = np.stack([np.stack([np.convolve(r, W, "same") for W in Ws])
                          for r in x.astype(np.float32).astype(np.float64)])
        check(got32, ref32[..., ::decim], 1, TOL32, f"cwt decim={decim} float32")
    flipped = np.stack([np.stack([np.convolve(r, W[::-1], "same") for W in Ws]) for r in x])
    assert errors(isd.tfr.cwt(x, Ws), flipped, 1)[0] > 0.1          # the test can tell the directions apart


# ---------------------------------------------------------------------------------------------------- type rules
def test_type_rules(isd):
    x, xd = case_data("A", torch.float64)
    for output in ("complex", "power", "phase", "avg_power", "itc", "avg_power_itc"):
        got = call(isd, x, "A", output=output)
        want = np.complex128 if output in ("complex", "avg_power_itc") else np.float64
        assert isinstance(got, np.ndarray) and got.dtype == want
        assert np.array_equal(got, call(isd, xd, "A", output=output).cpu().numpy())
    assert call(isd, x.astype(np.float32), "A", output="power").dtype == np.float64   # any float array: fp64
    _, x32 = case_data("A", torch.float32)
    for output in ("complex", "power", "phase", "avg_power", "itc", "avg_power_itc"):
        got = call(isd, x32, "A", output=output)
        want = torch.complex64 if output in ("complex", "avg_power_itc") else torch.float32
        assert got.dtype == want and got.device == x32.device
    for dtype, _ in DTYPES:
        _, xd = case_data("A", dtype)                               # (3, 2, 96)
        wide = torch.zeros(3, 2, 2 * 96, dtype=dtype, device="cuda")
        wide[..., ::2] = xd
        view = wide[..., ::2]
        assert not view.is_contiguous()
        assert torch.equal(call(isd, view, "A", output="power"), call(isd, xd, "A", output="power"))
        swapped = xd.transpose(0, 1)                                # (2, 3, 96), non-contiguous
        assert torch.equal(call(isd, swapped, "A"), call(isd, xd, "A").transpose(0, 1))
        empty = call(isd, xd[:0], "A", output="power")
        assert tuple(empty.shape) == (0, 2, 5, 96) and empty.dtype == dtype
        with pytest.raises(ValueError, match="n=0"):
            call(isd, xd[:0], "A", output="itc")
    with pytest.raises(TypeError):
        call(isd, xd.cpu(), "A")


# ------------------------------------------------------------------------------------- no access outside the data
def fenced(x, dtype, shift):
    """x as a contiguous view into a larger NaN-filled device buffer: NaN directly before its first and after its
    last row.  shift = 1 moves the block off its 16-byte alignment."""
    pad = 64
    buf = torch.full((x.size + 2 * pad + shift,), float("nan"), dtype=dtype, device="cuda")
    view = buf[pad + shift:pad + shift + x.size].view(x.shape)
    view.copy_(torch.tensor(x))
    return buf, view


@pytest.mark.parametrize("case", ["A", "C", "D", "F"])
def test_reads_nothing_outside_x(isd, case):
    for dtype, _ in DTYPES:
        x, xd = case_data(case, dtype)
        for output in ("complex", "avg_power_itc"):
            clean = call(isd, xd, case, output=output)
            for shift in (0, 1):
                buf, view = fenced(x, dtype, shift)
                got = call(isd, view, case, output=output)
                assert torch.isfinite(torch.view_as_real(got)).all() and torch.equal(got, clean), (dtype, output, shift)
                assert torch.isnan(buf[:64]).all() and torch.isnan(buf[-64:]).all()


@pytest.mark.parametrize("case", ["A", "D", "F"])
def test_writes_nothing_outside_out(isd, case):
    """Through the plan: the output is a view into a canary-filled buffer, 3 elements off its start."""
    _, sfreq, freqs, n_cycles = CASES[case]
    Ws = isd.tfr.morlet(sfreq, freqs, n_cycles, zero_mean=True)
    for decim in (1, 3):
        plan = isd.tfr.TfrPlan([len(W) for W in Ws], np.concatenate(Ws), decim)
        for dtype, _ in DTYPES:
            _, xd = case_data(case, dtype)
            for mode in isd.tfr.MODES:
                clean = plan(xd, mode)
                pad, canary = 67, -777.25
                buf = torch.full((clean.numel() + 2 * pad,), canary, dtype=clean.dtype, device="cuda")
                out = buf[pad:pad + clean.numel()].view(clean.shape)
                got = plan(xd, mode, out=out)
                assert got.data_ptr() == out.data_ptr() and torch.equal(out, clean), (dtype, mode, decim)
                assert bool((buf[:pad] == canary).all()) and bool((buf[-pad:] == canary).all()), (dtype, mode, decim)


# --------------------------------------------------------------------------------------- repeatability, memory
def test_two_calls_give_the_same_bits(isd):
    for dtype, _ in DTYPES:
        _, xd = case_data("F", dtype)
        for output in ("complex", "power", "phase", "avg_power", "itc", "avg_power_itc"):
            assert torch.equal(call(isd, xd, "F", output=output), call(isd, xd, "F", output=output)), (dtype, output)


def test_averaged_route_writes_nothing_per_trial(isd):
    _, sfreq, freqs, n_cycles = CASES["B"]
    x = torch.tensor(tfr_ref.make_data((16, 3, 300), sfreq), dtype=torch.float32).cuda()
    isd.tfr_array_morlet(x, sfreq, freqs, n_cycles, output="avg_power")        # the plan exists from here on
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = isd.tfr_array_morlet(x, sfreq, freqs, n_cycles, output="avg_power")
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    result = got.numel() * got.element_size()
    print(f"avg_power of (16, 3, 300): peak rise {rise} bytes for a result of {result} bytes")
    assert tuple(got.shape) == (3, 17, 300) and rise < 4 * result   # a per-trial power map would be 16 x, complex 32 x


# ------------------------------------------------------------------------------------------- the library's refusals
def test_library_refusals(isd):
    from isd_amd import _lib
    L = _lib.lib()

    def create(n_taps, decim, taps=True, out=True):
        h = C.c_void_p()
        n = max(sum(n_taps), 1)
        t = (C.c_double * (2 * n))(*([0.5] * (2 * n))) if taps else None
        rc = L.isd_tfr_plan_create(C.byref(h) if out else None, len(n_taps), _lib.int_array(n_taps), t, decim)
        msg = L.isd_last_error()
        if rc == 0:
            L.isd_tfr_plan_destroy(h)
        return rc, msg

    refused = (_lib.ISD_ERR_UNSUPPORTED, _lib.ISD_ERR_INVALID)
    for args, word in ((([5, 8], 1), b"n_taps[1]=8"), (([4097], 1), b"4097"), (([5], 0), b"decim=0"),
                       (([5], isd.tfr.MAX_DECIM + 1), b"decim"), (([1] * (isd.tfr.MAX_FREQS + 1), 1), b"n_freqs"),
                       (([], 1), b"n_freqs")):
        rc, msg = create(*args)
        assert rc in refused and word in msg, (args, rc, msg)
    for kw in ({"taps": False}, {"out": False}):
        rc, msg = create([5], 1, **kw)
        assert rc in refused and b"null" in msg, (kw, rc, msg)
    assert create([4095, 1], isd.tfr.MAX_DECIM)[0] == 0             # the corners of the envelope
    plan = isd.tfr.TfrPlan([5], np.ones(5, dtype=complex), 3)
    assert L.isd_tfr_plan_out_len(plan._h, 96) == 32 and L.isd_tfr_plan_out_len(plan._h, 97) == 33
    assert plan.useful_taps == 5 and plan.padded_taps == 8 * 16
    x = torch.zeros(2, 2, 96, device="cuda")
    out = torch.zeros(2, 2, 1, 32, device="cuda")
    work = torch.zeros(256, dtype=torch.uint8, device="cuda")
    for args in ((None, out.data_ptr(), 2, 2, 96, 1), (x.data_ptr(), None, 2, 2, 96, 1),
                 (x.data_ptr(), out.data_ptr(), 2, 2, 96, 6), (x.data_ptr(), out.data_ptr(), 0, 2, 96, 2),
                 (x.data_ptr(), out.data_ptr(), -1, 2, 96, 1)):
        rc = L.isd_tfr_cwt_f32(plan._h, args[0], args[1], args[2], args[3], args[4], args[5], work.data_ptr(), None)
        assert rc in refused and L.isd_last_error(), args
    assert L.isd_tfr_cwt_f32(None, x.data_ptr(), out.data_ptr(), 2, 2, 96, 1, work.data_ptr(), None) in refused
    torch.cuda.synchronize()
    assert bool((out == 0).all())                                   # none of them launched anything
