"""isd_amd.pac on the GPU against the NumPy float64 restatement of tests/pac_ref.py (itself pinned by closed forms in
test_pac_cpu.py).

The kernel tests feed phi and a directly (pac.pac_launch), rounded to the tested precision and widened again for the
reference, so no filter or FFT rounding is in the comparison, and ask for every surrogate value.  The error of a method
is the largest absolute error of a value: the estimate, every surrogate, the surrogate mean and std.

Bounds: an error above DEFECT (1e-5 fp32, 1e-12 fp64) is a defect whatever else holds; it is a priori (a CPU emulation
of sequential fp32 sums on these inputs gives 7e-8 mvl, 1.2e-7 mi and 7e-7 hr, so 1e-5 separates rounding from a wrong
index).  Below it, TOL per (precision, method) is 8 x the worst error observed on an MI355X, rounded up to one digit:
the kernel is bitwise repeatable, so the margin covers other clocks and library versions of sincos / log only.

Observed on an MI355X (worst over the ten cases, the scale test and the end-to-end test; each test prints its own):
  mvl   1.3e-15 fp64 (case 8)   4.0e-7 fp32 (case 8)
  mi    4.2e-16 fp64 (case 9)   3.1e-8 fp32 (case 9)
  hr    7.7e-16 fp64 (case 5)   3.2e-7 fp32 (case 4)
  case 1 x 1e-6: mvl 1.7e-16 / 8.2e-8, mi 3.9e-16 / 1.3e-8, hr exactly 1
  end to end (8 x 2 x 795, 32 surrogates): mvl 2.3e-16 / 9.2e-8, mi 4.1e-16 / 7.6e-9, hr 1.4e-16 / 2.7e-7
The fp32 mvl figure is above the 7e-8 of the CPU emulation of sequential sums because the kernel's sums run in
bin-sorted order, not in time order, and the figure is the worst of every shift and the surrogate statistics; it is
25 times below DEFECT.

n_ge must equal the reference's count wherever the reference's smallest |v(s_i) - v(0)| of the case exceeds 100 x TOL;
cases 1, 3 and 4 must have that gap (their seeds were picked for it on the CPU), except 'hr' of case 1, which is
exactly 1 throughout because 37 samples leave some of 18 bins empty: there the values and the count are asserted
exactly.
"""
import numpy as np
import pytest
import torch

from pac_ref import CASES, GAP_CASES, METHODS, make_case, min_gap, ref_block

pytestmark = pytest.mark.gpu

PRECISIONS = [(torch.float64, np.float64, "fp64"), (torch.float32, np.float32, "fp32")]
DEFECT = {"fp64": 1e-12, "fp32": 1e-5}
OBSERVED = {                         # (precision, method) -> worst error observed on an MI355X
    ("fp64", "mvl"): 1.25e-15, ("fp64", "mi"): 4.16e-16, ("fp64", "hr"): 7.63e-16,
    ("fp32", "mvl"): 3.91e-7, ("fp32", "mi"): 3.03e-8, ("fp32", "hr"): 3.11e-7,
}
TOL = {                              # 8 x OBSERVED, rounded up to one digit
    ("fp64", "mvl"): 1e-14, ("fp64", "mi"): 4e-15, ("fp64", "hr"): 7e-15,
    ("fp32", "mvl"): 4e-6, ("fp32", "mi"): 3e-7, ("fp32", "hr"): 3e-6,
}
_CACHE = {}


@pytest.fixture(scope="module")
def isd():
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd


def case_data(case, prec):
    """-> (pha, amp, shifts, B, block, surr): the inputs as the reference sees them and the reference, read-only."""
    key = (case, prec)
    if key not in _CACHE:
        npdtype = np.float64 if prec == "fp64" else np.float32
        pha, amp, shifts, B = make_case(case, npdtype)
        block, surr = ref_block(pha, amp, shifts, B)
        for a in (pha, amp, shifts, block, surr):
            a.setflags(write=False)
        _CACHE[key] = (pha, amp, shifts, B, block, surr)
    return _CACHE[key]


def launch(isd, pha, amp, shifts, B, tdtype):
    out, surr = isd.pac.pac_launch(torch.tensor(pha, dtype=tdtype).cuda(), torch.tensor(amp, dtype=tdtype).cuda(),
                                   np.array(shifts), B, surrogates_out=True)
    assert out.is_cuda and out.dtype == tdtype and surr.dtype == tdtype
    return out, surr


def method_errors(got, got_surr, block, surr, scale=(1.0, 1.0, 1.0)):
    """-> [3]: the largest |error| per method over the estimate, the surrogates, their mean and their std; the
    kernel's values are multiplied by ``scale`` per method first.  NaN must sit where the reference has it (the
    surrogate mean and std without surrogates)."""
    errs = []
    for m in range(3):
        g = np.concatenate([got[..., m, :3].reshape(-1), got_surr[..., m, :].reshape(-1)]) * scale[m]
        r = np.concatenate([block[..., m, :3].reshape(-1), surr[..., m, :].reshape(-1)])
        assert np.array_equal(np.isnan(g), np.isnan(r)), METHODS[m]
        ok = ~np.isnan(r)
        errs.append(float(np.abs(g - r)[ok].max()))
    return errs


def check(failures, what, err, prec, method):
    if err > DEFECT[prec]:
        failures.append(f"{what} {prec} {method}: {err:.2e} is above {DEFECT[prec]:g}: a defect, not a tolerance")
    elif err > TOL[(prec, method)]:
        failures.append(f"{what} {prec} {method}: {err:.2e} > {TOL[(prec, method)]:g}")


# ------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("case", sorted(CASES))
def test_matches_the_restatement(isd, case):
    failures = []
    k = CASES[case]
    for tdtype, _, prec in PRECISIONS:
        pha, amp, shifts, B, block, surr = case_data(case, prec)
        out, sur = launch(isd, pha, amp, shifts, B, tdtype)
        assert tuple(out.shape) == (k["rows"], k["A"], k["P"], 3, 4) == block.shape
        assert tuple(sur.shape) == (k["rows"], k["A"], k["P"], 3, k["S"]) == surr.shape
        got, got_surr = out.cpu().numpy().astype(np.float64), sur.cpu().numpy().astype(np.float64)
        errs = method_errors(got, got_surr, block, surr)
        gaps = min_gap(block, surr) if k["S"] else [np.inf] * 3
        for m, name in enumerate(METHODS):
            print(f"case {case} {prec} {name}: max |err| = {errs[m]:.2e}  smallest |v(s_i) - v(0)| = {gaps[m]:.2e}")
            check(failures, f"case {case}", errs[m], prec, name)
            exactly_one = case == 1 and name == "hr"
            if exactly_one:                                              # empty bins: 1 everywhere, in any precision
                assert (block[..., m, 0] == 1).all() and (surr[..., m, :] == 1).all()
                assert (got[..., m, 0] == 1).all() and (got_surr[..., m, :] == 1).all()
            elif case in GAP_CASES and not gaps[m] > 100 * TOL[(prec, name)]:
                failures.append(f"case {case} {prec} {name}: the reference's gap {gaps[m]:.2e} is not above "
                                f"100 x {TOL[(prec, name)]:g}")
            if exactly_one or gaps[m] > 100 * TOL[(prec, name)]:
                if not np.array_equal(got[..., m, 3], block[..., m, 3]):
                    failures.append(f"case {case} {prec} {name}: n_ge differs from the reference's count")
    assert not failures, failures


def test_two_calls_give_the_same_bits(isd):
    for tdtype, _, prec in PRECISIONS:
        pha, amp, shifts, B, _, _ = case_data(4, prec)
        a, b = launch(isd, pha, amp, shifts, B, tdtype), launch(isd, pha, amp, shifts, B, tdtype)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        pd, ad = torch.tensor(pha, dtype=tdtype).cuda(), torch.tensor(amp, dtype=tdtype).cuda()
        only = isd.pac.pac_launch(pd, ad, np.array(shifts), B)           # without the surrogate values
        assert torch.equal(only, a[0])
        dev = isd.pac.pac_launch(pd, ad, torch.tensor(np.array(shifts)).cuda(), B)       # shifts on the device
        assert torch.equal(dev, a[0])


def test_microvolt_scale(isd):
    failures = []
    for tdtype, npdtype, prec in PRECISIONS:
        pha, amp, shifts, B, block, surr = case_data(1, prec)
        out, sur = launch(isd, pha, (amp * 1e-6).astype(npdtype), shifts, B, tdtype)
        errs = method_errors(out.cpu().numpy().astype(np.float64), sur.cpu().numpy().astype(np.float64), block, surr,
                             scale=(1e6, 1.0, 1.0))
        for m, name in enumerate(METHODS):
            print(f"case 1 x 1e-6 {prec} {name}: max |err| = {errs[m]:.2e}")
            check(failures, "case 1 x 1e-6", errs[m], prec, name)
    assert not failures, failures


@pytest.mark.parametrize("case", [1, 3, 6])
def test_nan_fences_around_the_inputs_change_nothing(isd, case):
    for tdtype, _, prec in PRECISIONS:
        pha, amp, shifts, B, _, _ = case_data(case, prec)
        clean = launch(isd, pha, amp, shifts, B, tdtype)
        for shift in (1, 3):
            views = []
            for a in (pha, amp):
                buf = torch.full((a.size + 128 + shift,), float("nan"), dtype=tdtype, device="cuda")
                v = buf[64 + shift:64 + shift + a.size].view(a.shape)
                v.copy_(torch.tensor(a, dtype=tdtype))
                views.append(v)
            got = isd.pac.pac_launch(views[0], views[1], np.array(shifts), B, surrogates_out=True)
            assert torch.isfinite(got[0]).all() and torch.equal(got[0], clean[0]) and torch.equal(got[1], clean[1])


# ------------------------------------------------------------------------------------------------------- end to end
FS, F_PHA, F_AMP, EDGES, N_SURR = 250.0, [(4, 8), (13, 20)], [(30, 50), (60, 90)], 50, 32


def coupled_trials():
    """[8, 2, 795]: channel 0 a 6 Hz sinusoid whose phase modulates a 40 Hz component, channel 1 the same components
    unmodulated; 0.3 sigma noise on both."""
    if "x" not in _CACHE:
        rng = np.random.default_rng(21)
        t = np.arange(795) / FS
        phi = 2 * np.pi * 6.0 * t[None, :] + rng.uniform(0, 2 * np.pi, (8, 1))
        fast = 0.3 * np.sin(2 * np.pi * 40.0 * t)[None, :]
        x = np.stack([np.sin(phi) + (1.0 + 0.8 * np.sin(phi)) * fast, np.sin(phi) + fast], 1)
        x = x + 0.3 * rng.standard_normal(x.shape)
        x.setflags(write=False)
        _CACHE["x"] = x
    return _CACHE["x"]


def end_to_end_reference(isd, xd):
    """ref_block of the package's own FirFilter + hilbert outputs (angle and abs taken by torch on the device, so the
    kernel and the reference bin the same numbers), pulled to the CPU -> (block [8, 2, A, P, 3, 4], shifts)."""
    n, Cc, T = xd.shape
    parts = []
    for lo, hi in F_PHA + F_AMP:
        z = isd.hilbert(isd.FirFilter(FS, lo, hi)(xd))[..., EDGES:T - EDGES]
        parts.append((torch.angle(z) if (lo, hi) in F_PHA else z.abs()).cpu().numpy().astype(np.float64))
    pha = np.stack(parts[:len(F_PHA)], 2).reshape(n * Cc, len(F_PHA), -1)
    amp = np.stack(parts[len(F_PHA):], 2).reshape(n * Cc, len(F_AMP), -1)
    shifts = isd.pac.draw_shifts(T - 2 * EDGES, N_SURR, 0)
    block, surr = ref_block(pha, amp, shifts, 18)
    return block.reshape(n, Cc, len(F_AMP), len(F_PHA), 3, 4), surr.reshape(n, Cc, len(F_AMP), len(F_PHA), 3, N_SURR)


@pytest.mark.parametrize("route", ["fp32", "ndarray"])
def test_end_to_end(isd, route, monkeypatch):
    x = coupled_trials()
    prec = "fp32" if route == "fp32" else "fp64"
    xd = torch.tensor(x, dtype=torch.float32 if route == "fp32" else torch.float64).cuda()
    arg = xd if route == "fp32" else np.array(x)
    kw = dict(sfreq=FS, f_pha=F_PHA, f_amp=F_AMP, edges=EDGES, n_surrogates=N_SURR, random_state=0)
    block, surr = end_to_end_reference(isd, xd)
    as_np = (lambda a: a.cpu().numpy()) if route == "fp32" else (lambda a: a)

    failures = []
    res = isd.phase_amplitude_coupling(arg, method=list(METHODS), return_stats=True, **kw)
    gaps = min_gap(block.reshape(-1, 1, 1, 3, 4), surr.reshape(-1, 1, 1, 3, N_SURR))
    for m, name in enumerate(METHODS):
        r = res[m]
        for f in r:
            if route == "fp32":
                assert f.is_cuda and f.dtype == torch.float32 and tuple(f.shape) == (8, 2, 2, 2)
            else:
                assert isinstance(f, np.ndarray) and f.dtype == np.float64 and f.shape == (8, 2, 2, 2)
        err = max(float(np.abs(as_np(f).astype(np.float64) - block[..., m, i]).max())
                  for i, f in enumerate((r.pac, r.surr_mean, r.surr_std)))
        print(f"end to end {route} {name}: max |err| = {err:.2e}  smallest gap = {gaps[m]:.2e}")
        check(failures, "end to end", err, prec, name)
        if gaps[m] > 100 * TOL[(prec, name)]:
            assert np.array_equal(as_np(r.pvalues), ((1.0 + block[..., m, 3]) / (1.0 + N_SURR)).astype(as_np(r.pvalues).dtype))
        single = isd.phase_amplitude_coupling(arg, method=name, **kw)             # a list is the single calls, bitwise
        assert np.array_equal(as_np(single), as_np(r.pac))
        z = isd.phase_amplitude_coupling(arg, method=name, normalize="zscore", **kw)
        assert np.array_equal(as_np(z), as_np((r.pac - r.surr_mean) / r.surr_std), equal_nan=True)
    assert not failures, failures

    mi = as_np(res[1].pac)                                                # [n, C, A, P]: the coupled entry wins
    for i in range(8):
        assert np.argmax(mi[i].reshape(-1)) == 0, mi[i]
        others = np.sort(mi[i].reshape(-1))[::-1]
        print(f"trial {i}: coupled MI {others[0]:.4f}, next {others[1]:.4f}")

    two = isd.phase_amplitude_coupling(arg, method=["mi", "mvl"], **kw)
    assert np.array_equal(as_np(two[0]), as_np(res[1].pac)) and np.array_equal(as_np(two[1]), as_np(res[0].pac))

    es = 4 if route == "fp32" else 8                                      # three trials per chunk: 3 + 3 + 2
    monkeypatch.setattr(isd.pac, "PAC_CHUNK_BYTES", 3 * isd.pac.trial_bytes(2, 2, 2, 695, 795, es) + 1)
    chunked = isd.phase_amplitude_coupling(arg, method=list(METHODS), return_stats=True, **kw)
    for a, b in zip(chunked, res):
        for fa, fb in zip(a, b):
            assert np.array_equal(as_np(fa), as_np(fb), equal_nan=True)
    one = isd.phase_amplitude_coupling(arg[3], method="mi", **kw)         # [C, T] is n = 1
    assert tuple(one.shape) == (2, 2, 2) and np.array_equal(as_np(one), as_np(res[1].pac)[3])
