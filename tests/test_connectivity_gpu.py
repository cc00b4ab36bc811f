"""isd_amd.connectivity on the GPU against the NumPy float64 restatement of tests/test_connectivity_cpu.py (ref_csd,
ref_measures; itself pinned by scipy.signal.csd / coherence there), over CASES of that file.

Data: test_psd_cpu.make_data (noise + a common 10 Hz line + per-row offsets 0 / 50 / -200).  For float32 the reference
sees the float32-rounded input widened to float64.  CSD bounds: the largest absolute error over the reference's largest
magnitude <= TOL64 = 1e-12 / TOL32 = 1e-5 (the bounds of test_psd_gpu.py).

Measure bounds (absolute error; MEASURE_TOL) are 8 x the worst error observed on an MI355X per measure and precision,
rounded up to one digit: the kernels are bitwise repeatable, so the margin covers other clocks and operator orders of
the elementwise torch step only.  An observed error above 1e-4 (fp32) / 1e-10 (fp64) counts as a defect, not a
tolerance, and fails whatever MEASURE_TOL says.  'ciplv' is compared where the reference's 1 - (Re E)^2 is at least
1e-6, off the diagonal and off the DC and Nyquist bins (every spectrum is real there, E is a mean of +-1 and ciplv is
0 / 0 as on the diagonal); what the cut-off then drops must stay under 1 % of the entries (2 % for s1 per trial, where the
restatement alone drops 1.4 %).  'ciplv' is asked for in a call of its own: a call that holds it runs its unit-modulus pass in fp64
whatever the input type, and 'plv' / 'ppc' are to be measured on the fp32 kernels.

Observed on an MI355X (worst over the cases; each test prints its own figures):
  csd, fp64      1.0e-14 (big, per trial)     diagonal against psd_array_welch 4.8e-16
  csd, fp32      6.0e-7  (s1, per trial)      diagonal against psd_array_welch 2.6e-7
  taps / remove_dc=False (case b)   3.1e-15 / 4.2e-16 fp64,  1.5e-7 / 2.8e-7 fp32;  five trial chunks: as one chunk
  coh / cohy     3.8e-12 fp64,  4.3e-6 fp32   imcoh 5.6e-13 / 1.3e-6     (all: big, per trial, N = 3)
  plv            9.6e-12 fp64,  5.3e-6 fp32   ppc   2.2e-11 / 8.8e-6
  coh^2 against scipy.signal.coherence (case b)   7.4e-15 fp64,  6.3e-7 fp32;   CoSpectra 9.2e-16 / 2.3e-7
  282 x 128 x 64 over trials in chunks of 170 + 112   1.7e-15 fp64,  2.5e-7 fp32
  E of s1 scaled by 2^-600 (fp64) / 2^-80 (fp32)      2.3e-15 / 7.0e-7, as unscaled
  ciplv          fp64: 8.8e-11 (s1 per trial), 4.5e-11 (big per trial), <= 1.4e-12 elsewhere
                 fp32: 3.0e-8 everywhere, half a unit in the last place of a float32 near 1

ciplv = |Im E| / sqrt(d), d = 1 - (Re E)^2, moves by up to e / sqrt(d) + e / d for an error e in E, and the compared
entries reach down to d = 1.6e-6 (s1 per trial: S = 1 makes |E| = 1 and the common 10 Hz line aligns the phases),
1.5e-5 (big per trial, N = 3) and 2.4e-4 (s1 over trials).  From a float32 E (e up to 5.6e-6) that gave 3.0e-2, 1.2e-3
and 2.4e-4, which is why the pass behind ciplv is fp64.  In fp64 the restatement's own distance from the exact value
(1 wherever S = 1) is 4.8e-11 on s1 per trial, so 8.8e-11 there is the two roundings together, close under the line.
E itself is held to the rounding of each spectrum over its modulus (phase_bound) on the fp32 and the fp64 kernels,
and the error of ciplv times d to twice that (test_phase_product_and_the_conditioning_of_ciplv).
"""
import ctypes as C

import numpy as np
import pytest
import scipy.signal as ss
import torch

from test_connectivity_cpu import CASES, ref_csd, ref_measures
from test_psd_cpu import ASYM_TAPS, make_data

pytestmark = pytest.mark.gpu

TOL64, TOL32 = 1e-12, 1e-5
DTYPES = [(torch.float64, TOL64), (torch.float32, TOL32)]
DEFECT = {torch.float64: 1e-10, torch.float32: 1e-4}
# worst observed absolute error per measure on an MI355X: (fp64, fp32), with the case that gave it
OBSERVED = {
    "coh": (3.84e-12, 4.29e-6),      # big, per trial
    "cohy": (3.84e-12, 4.29e-6),     # big, per trial
    "imcoh": (5.60e-13, 1.28e-6),    # big / a, per trial
    "plv": (9.59e-12, 5.26e-6),      # big, per trial (N = 3)
    "ciplv": (8.82e-11, 2.98e-8),    # s1, per trial / fp32: the result's own rounding (its pass is fp64)
    "ppc": (2.22e-11, 8.76e-6),      # big, per trial
}
MEASURE_TOL = {                      # 8 x OBSERVED, rounded up to one digit
    "coh": (4e-11, 4e-5), "cohy": (4e-11, 4e-5), "imcoh": (5e-12, 2e-5),
    "plv": (8e-11, 5e-5), "ciplv": (8e-10, 3e-7), "ppc": (2e-10, 8e-5),
}
METHODS = ["coh", "cohy", "imcoh", "plv", "ciplv", "ppc"]
_REFS = {}


@pytest.fixture(scope="module")
def isd():
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd


def case_data(case, dtype):
    key = ("x", case, dtype)
    if key not in _REFS:
        shape, sfreq = CASES[case][:2]
        x = make_data(shape, sfreq)
        if dtype == torch.float32:
            x = x.astype(np.float32).astype(np.float64)
        x.setflags(write=False)
        _REFS[key] = x
    x = _REFS[key]
    return x, torch.tensor(x, dtype=dtype).cuda()


def reference(case, dtype, average, window="hann", remove_dc=True, unit_modulus=False):
    key = ("csd", case, dtype, average, window if isinstance(window, str) else "taps", remove_dc, unit_modulus)
    if key not in _REFS:
        x, _ = case_data(case, dtype)
        S, f, N = ref_csd(x, *CASES[case][1:], window, remove_dc, average, unit_modulus)
        S.setflags(write=False)
        _REFS[key] = (S, f, N)
    return _REFS[key]


def kw(case, **more):
    _, sfreq, n_fft, nps, nov, fmin, fmax = CASES[case]
    return dict(sfreq=sfreq, fmin=fmin, fmax=fmax, n_fft=n_fft, n_overlap=nov, n_per_seg=nps, **more)


def _err(got, ref):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return float(np.abs(got.astype(np.complex128) - ref).max() / np.abs(ref).max())


def check_structure(S):
    assert torch.equal(S, S.transpose(-1, -2).conj().resolve_conj())
    assert (torch.diagonal(S, dim1=-2, dim2=-1).imag == 0).all()


# ------------------------------------------------------------------------------------------------------ the density
@pytest.mark.parametrize("average", ["segments", "trials"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_csd_matches_the_restatement(isd, case, average):
    for dtype, tol in DTYPES:
        _, xd = case_data(case, dtype)
        ref, f, _ = reference(case, dtype, average)
        got, freqs = isd.connectivity.csd_array_welch(xd, average=average, **kw(case))
        assert got.is_cuda and got.dtype == (torch.complex128 if dtype == torch.float64 else torch.complex64)
        assert tuple(got.shape) == ref.shape and np.array_equal(freqs, f) and freqs.dtype == np.float64
        err = _err(got, ref)
        print(f"case {case} {average} {str(dtype)[6:]}: max|err|/max|ref| = {err:.2e}")
        assert err <= tol
        check_structure(got)
        psd = isd.psd_array_welch(xd, window="hann", **kw(case))[0]             # [n, C, K]
        dg = torch.diagonal(got, dim1=-2, dim2=-1).real                       # [(n,) K, C]
        want = psd.transpose(-1, -2) if average == "segments" else psd.mean(0).transpose(-1, -2)
        derr = float((dg - want).abs().max() / want.abs().max())
        print(f"case {case} {average} {str(dtype)[6:]}: diagonal against psd_array_welch = {derr:.2e}")
        assert derr <= tol


@pytest.mark.parametrize("window", ["hann", "taps"])
@pytest.mark.parametrize("remove_dc", [True, False])
def test_case_b_windows_and_remove_dc(isd, window, remove_dc):
    w = ASYM_TAPS if window == "taps" else window
    for dtype, tol in DTYPES:
        _, xd = case_data("b", dtype)
        for average in ("segments", "trials"):
            ref = reference("b", dtype, average, w, remove_dc)[0]
            got = isd.connectivity.csd_array_welch(xd, average=average, window=w, remove_dc=remove_dc, **kw("b"))[0]
            err = _err(got, ref)
            print(f"case b {window} remove_dc={remove_dc} {average} {str(dtype)[6:]}: {err:.2e}")
            assert err <= tol
            check_structure(got)


def test_c1_is_the_psd(isd):
    for dtype, tol in DTYPES:
        _, xd = case_data("c1", dtype)
        got = isd.connectivity.csd_array_welch(xd, **kw("c1"))[0]                # [2, 33, 1, 1]
        psd = isd.psd_array_welch(xd, window="hann", **kw("c1"))[0]              # [2, 1, 33]
        assert (got.imag == 0).all()
        assert float((got.real[:, :, 0, 0] - psd[:, 0]).abs().max() / psd.abs().max()) <= tol


def test_two_calls_and_views_give_the_same_bits(isd):
    for dtype, _ in DTYPES:
        for case in ("a", "big", "c"):
            _, xd = case_data(case, dtype)
            for average in ("segments", "trials"):
                a = isd.connectivity.csd_array_welch(xd, average=average, **kw(case))[0]
                b = isd.connectivity.csd_array_welch(xd, average=average, **kw(case))[0]
                assert torch.equal(a, b), (case, average, dtype)
        _, xd = case_data("a", dtype)
        base = isd.connectivity.csd_array_welch(xd, **kw("a"))[0]
        wide = torch.zeros(3, 5, 2 * 795, dtype=dtype, device="cuda")
        wide[..., ::2] = xd
        view = wide[..., ::2]
        assert not view.is_contiguous()
        assert torch.equal(isd.connectivity.csd_array_welch(view, **kw("a"))[0], base)
        one = isd.connectivity.csd_array_welch(xd[1], **kw("a"))[0]                   # [C, T] is n = 1
        assert tuple(one.shape) == (129, 5, 5) and torch.equal(one, base[1])


def test_ndarray_route_is_the_fp64_route(isd):
    x, xd = case_data("b", torch.float64)
    for average in ("segments", "trials"):
        got, freqs = isd.connectivity.csd_array_welch(x, average=average, **kw("b"))
        assert isinstance(got, np.ndarray) and got.dtype == np.complex128
        assert np.array_equal(got, isd.connectivity.csd_array_welch(xd, average=average, **kw("b"))[0].cpu().numpy())
    con, _ = isd.connectivity.spectral_connectivity(x.astype(np.float32), method=["coh", "cohy"], **kw("b"))
    assert con[0].dtype == np.float64 and con[1].dtype == np.complex128


def fenced(shape, dtype, shift):
    """A contiguous view of `shape` inside a larger NaN-filled device buffer, `shift` elements off its start."""
    pad, size = 64, int(np.prod(shape))
    nan = complex("nan+nanj") if dtype.is_complex else float("nan")
    buf = torch.full((size + 2 * pad + shift,), nan, dtype=dtype, device="cuda")
    return buf, buf[pad + shift:pad + shift + size].view(shape)


@pytest.mark.parametrize("case", ["a", "b", "c", "c65", "big"])
def test_nan_fences_around_x_and_out_stay_intact(isd, case):
    from isd_amd import connectivity as con
    for dtype, _ in DTYPES:
        x, xd = case_data(case, dtype)
        cdtype = torch.complex128 if dtype == torch.float64 else torch.complex64
        d = con._design(x.shape[-1], *[kw(case)[k] for k in ("sfreq", "fmin", "fmax", "n_fft", "n_overlap",
                                                               "n_per_seg")], "hann")
        plan = con._plan_for(d, kw(case)["sfreq"], True, xd.device)
        for over in (False, True):
            for unit in (False, True):
                clean = con.csd_launch(plan, xd, over, unit)
                for shift in (0, 1):
                    xbuf, xv = fenced(x.shape, dtype, shift)
                    xv.copy_(xd)
                    obuf, ov = fenced(tuple(clean.shape), cdtype, shift)       # shifted by one complex element
                    got = con.csd_launch(plan, xv, over, unit, out=ov)
                    assert got.data_ptr() == ov.data_ptr()
                    assert torch.isfinite(torch.view_as_real(got)).all() and torch.equal(got, clean)
                    for buf in (xbuf, torch.view_as_real(obuf)):
                        assert torch.isnan(buf[:64]).all() and torch.isnan(buf[-64:]).all(), (dtype, over, unit, shift)


def test_over_trials_split_reduce_and_trial_chunks(isd):
    """case big: 33 bins x one tile pair is too few waves, so the 900 (trial, segment) pairs are split into ranges and
    reduced; a small chunk budget then runs the trials in several chunks inside the call."""
    from isd_amd import connectivity as con
    for dtype, tol in DTYPES:
        _, xd = case_data("big", dtype)
        refs = {a: reference("big", dtype, a)[0] for a in ("segments", "trials")}
        whole = {a: con.csd_array_welch(xd, average=a, **kw("big"))[0] for a in refs}
        per_trial = 4 * 3 * 8 + 33 * 2 * 3 * 4 * xd.element_size()
        try:
            con.CSD_CHUNK_BYTES = 64 * per_trial                               # 300 trials in chunks of 64 (last: 44)
            for a, ref in refs.items():
                got = con.csd_array_welch(xd, average=a, **kw("big"))[0]
                err = _err(got, ref)
                print(f"case big {a} {str(dtype)[6:]} in 5 chunks: {err:.2e}")
                assert err <= tol
                check_structure(got)
                if a == "segments":
                    assert torch.equal(got, whole[a])                          # per trial: chunks change nothing
                assert torch.equal(got, con.csd_array_welch(xd, average=a, **kw("big"))[0])
        finally:
            con.CSD_CHUNK_BYTES = None
        assert torch.equal(con.csd_array_welch(xd, average="trials", **kw("big"))[0], whole["trials"])


def test_short_last_chunk_has_no_more_ranges_than_a_full_one(isd):
    """C = 128, K = 33: 297 product workgroups, at most 14 ranges.  Chunks of 170 trials (S = 1: 170 pairs, 11 ranges
    of 16) leave a last chunk of 112, which split on its own would be 14 ranges of 8, three more than the partial
    sums of a full chunk have room for; it is cut into ranges of 16 like the others."""
    from isd_amd import connectivity as con
    shape, args = (282, 128, 64), dict(sfreq=128.0, n_fft=64, n_per_seg=64, n_overlap=0)
    x = make_data(shape, 128.0)
    ref = ref_csd(x, 128.0, 64, 64, 0, 0.0, np.inf, average="trials")[0]
    for dtype, tol in DTYPES:
        xr = x.astype(np.float32).astype(np.float64) if dtype == torch.float32 else x
        r = ref if dtype == torch.float64 else ref_csd(xr, 128.0, 64, 64, 0, 0.0, np.inf, average="trials")[0]
        xd = torch.tensor(xr, dtype=dtype).cuda()
        per_trial = 128 * 8 + 33 * 2 * 128 * xd.element_size()
        guard = torch.full((1 << 22,), float("nan"), dtype=dtype, device="cuda")       # next to `work`, if anything
        try:
            con.CSD_CHUNK_BYTES = 170 * per_trial
            got = con.csd_array_welch(xd, average="trials", **args)[0]
            again = con.csd_array_welch(xd, average="trials", **args)[0]
        finally:
            con.CSD_CHUNK_BYTES = None
        err = _err(got, r)
        print(f"282 trials in chunks of 170 + 112, {str(dtype)[6:]}: {err:.2e}")
        assert err <= tol and torch.equal(got, again) and torch.isnan(guard).all()
        check_structure(got)


def test_unit_modulus_of_spectra_whose_squares_underflow(isd):
    """x scaled by an exact power of two so small that |X|^2 underflows: the phase product must not change beyond
    rounding (only an exact zero stays zero)."""
    from isd_amd import connectivity as con
    for (dtype, tol), power in zip(DTYPES, (-600, -80)):
        _, xd = case_data("s1", dtype)                                          # every |X| within 0.79 of the largest
        E = reference("s1", dtype, "segments", unit_modulus=True)[0]
        plan = unit_plan("s1", xd)
        small = con.csd_launch(plan, xd * 2.0 ** power, False, unit_modulus=True)
        err = _err(small, E)
        print(f"case s1 {str(dtype)[6:]} x 2^{power}: E {err:.2e}")
        assert err <= tol
        check_structure(small)


# ----------------------------------------------------------------------------------------------------- the measures
def measure_errors(isd, case, dtype, average):
    x, xd = case_data(case, dtype)
    S, f, N = reference(case, dtype, average)
    E = reference(case, dtype, average, unit_modulus=True)[0]
    methods = [m for m in METHODS if not (m == "ppc" and N < 2)]
    ref = ref_measures(S, E, N)
    rest = [m for m in methods if m != "ciplv"]
    got, freqs = isd.connectivity.spectral_connectivity(xd, method=rest, average=average, **kw(case))
    assert np.array_equal(freqs, f)
    both = isd.connectivity.spectral_connectivity(xd, method=["ciplv", "plv"], average=average, **kw(case))[0]
    alone = isd.connectivity.spectral_connectivity(xd, method="ciplv", average=average, **kw(case))[0]
    assert both[0].dtype == xd.dtype and both[1].dtype == xd.dtype
    assert torch.equal(torch.nan_to_num(both[0]), torch.nan_to_num(alone))       # a list changes no bits of it
    got = dict(zip(rest, got), ciplv=alone)
    got = [got[m] for m in methods]
    Cc = S.shape[-1]
    off = ~np.eye(Cc, dtype=bool)
    errs = {}
    for m, g in zip(methods, got):
        g = g.cpu().numpy()
        assert g.shape == ref[m].shape and g.dtype.kind == ("c" if m == "cohy" else "f")
        mask = np.broadcast_to(off, g.shape).copy() if m == "ciplv" else np.ones(g.shape, dtype=bool)
        if m == "ciplv":
            k = np.rint(f * CASES[case][2] / CASES[case][1]).astype(int)
            real_bin = (k == 0) | (2 * k == CASES[case][2])          # DC and Nyquist: every spectrum is real, so
            mask[..., real_bin, :, :] = False                         # E is a mean of +-1 and ciplv can be 0 / 0
            ok = (1.0 - E.real ** 2) >= 1e-6
            dropped = float((mask & ~ok).sum()) / max(1, mask.sum())
            mask &= ok
            errs["ciplv_dropped"] = dropped
        errs[m] = float(np.abs(g.astype(np.complex128) - ref[m])[mask].max()) if mask.any() else 0.0
    return errs


@pytest.mark.parametrize("average", ["segments", "trials"])
@pytest.mark.parametrize("case", ["a", "b", "c", "s1", "c65", "c128", "big"])
def test_measures_match_the_restatement(isd, case, average):
    failures = []
    for i, (dtype, _) in enumerate(DTYPES):
        errs = measure_errors(isd, case, dtype, average)
        print(f"case {case} {average} {str(dtype)[6:]}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        dropped = errs.pop("ciplv_dropped")
        # S = 1 per trial makes every |E| 1 and the common 10 Hz line aligns the phases at the one kept bin: the
        # float64 restatement alone puts 10 of the 720 entries (1.4 %) under the cut-off there, so that case is held
        # to 2 %, every other to 1 %
        limit = 0.02 if (case == "s1" and average == "segments") else 0.01
        if dropped >= limit:
            failures.append(f"{str(dtype)[6:]}: ciplv compared on too few entries ({dropped:.1%} dropped)")
        for m, e in errs.items():
            if e > DEFECT[dtype]:
                failures.append(f"{str(dtype)[6:]} {m}: {e:.2e} is above {DEFECT[dtype]:g}: a defect, not a tolerance")
            elif e > MEASURE_TOL[m][i]:
                failures.append(f"{str(dtype)[6:]} {m}: {e:.2e} > {MEASURE_TOL[m][i]:g}")
    assert not failures, failures


def unit_plan(case, xd):
    from isd_amd import connectivity as con
    k = kw(case)
    d = con._design(xd.shape[-1], k["sfreq"], k["fmin"], k["fmax"], k["n_fft"], k["n_overlap"], k["n_per_seg"], "hann")
    return con._plan_for(d, k["sfreq"], True, xd.device)


def phase_bound(case, dtype, average, tol):
    """Elementwise bound on the error of E = mean_p u_i conj(u_j), u = X / |X|: a spectrum known to tol M (M the
    largest |X| of the case, the bound of the density applied to the spectra) gives u to tol M / |X|, and a product
    of two unit numbers moves by the sum of their errors: tol mean_p (M / |X_ip| + M / |X_jp|)."""
    from test_connectivity_cpu import ref_spectra
    key = ("phase_bound", case, dtype, average)
    if key not in _REFS:
        x, _ = case_data(case, dtype)
        X = np.abs(ref_spectra(x, *CASES[case][1:])[0])                       # [n, C, S, K]
        with np.errstate(divide="ignore"):
            inv = X.max() / X
        A = inv.mean(2).transpose(0, 2, 1) if average == "segments" else inv.mean((0, 2)).T     # [(n,) K, C]
        _REFS[key] = A[..., :, None] + A[..., None, :]
    return tol * _REFS[key]


@pytest.mark.parametrize("average", ["segments", "trials"])
@pytest.mark.parametrize("case", ["a", "c", "s1", "big"])
def test_phase_product_and_the_conditioning_of_ciplv(isd, case, average):
    """The mean phase product E is held to phase_bound, B.  With d = 1 - (Re E)^2 and |Im E| <= sqrt(d), an error e
    in E moves ciplv = |Im E| / sqrt(d) by at most e / sqrt(d) + e / d <= 2 e / d: the error of ciplv times d stays
    below 2 B wherever it is compared, however small d is."""
    from isd_amd import connectivity as con
    for dtype, tol in DTYPES:
        _, xd = case_data(case, dtype)
        E, f, N = reference(case, dtype, average, unit_modulus=True)
        B = phase_bound(case, dtype, average, tol)
        got = con.csd_launch(unit_plan(case, xd), xd, average == "trials", unit_modulus=True)
        check_structure(got)
        eerr = np.abs(got.cpu().numpy().astype(np.complex128) - E)
        ci = con.spectral_connectivity(xd, method="ciplv", average=average, **kw(case))[0].cpu().numpy()
        d = 1.0 - E.real ** 2
        mask = np.broadcast_to(~np.eye(E.shape[-1], dtype=bool), E.shape) & (d >= 1e-6)
        cerr = np.abs(ci - ref_measures(None, E, N)["ciplv"]) * d
        print(f"case {case} {average} {str(dtype)[6:]}: |E err| {eerr.max():.2e}, over its bound {(eerr / B).max():.2e}"
              f"   |ciplv err| d {cerr[mask].max():.2e}, over twice the bound {(cerr / (2 * B))[mask].max():.2e}"
              f"   min d {d[mask].min():.2e}")
        assert (eerr <= B).all() and (cerr[mask] <= 2 * B[mask]).all()


def test_s1_coherence_is_one_per_trial_and_not_over_trials(isd):
    for dtype, tol in DTYPES:
        _, xd = case_data("s1", dtype)
        per = isd.connectivity.spectral_connectivity(xd, method="coh", average="segments", **kw("s1"))[0]
        assert tuple(per.shape) == (3, 1, 16, 16)
        dev = float((per - 1).abs().max())
        print(f"case s1 {str(dtype)[6:]}: per-trial |coh - 1| = {dev:.2e}")
        assert dev <= tol
        over = isd.connectivity.spectral_connectivity(xd, method="coh", average="trials", **kw("s1"))[0]
        off = ~torch.eye(16, dtype=torch.bool, device="cuda")
        assert float(over[0][off].min()) < 0.999


def test_coh_squared_is_scipy_coherence_on_case_b(isd):
    shape, sfreq, n_fft, nps, nov, fmin, fmax = CASES["b"]
    for i, (dtype, _) in enumerate(DTYPES):
        x, xd = case_data("b", dtype)
        coh = isd.connectivity.spectral_connectivity(xd, method="coh", average="segments", **kw("b"))[0].cpu().numpy()
        fs_, c = ss.coherence(x[:, :, None, :], x[:, None, :, :], sfreq, window="hann", nperseg=nps, noverlap=nov,
                              nfft=n_fft, detrend="constant")
        c = c[..., (fs_ >= fmin) & (fs_ <= fmax)].transpose(0, 3, 1, 2)
        err = float(np.abs(coh.astype(np.float64) ** 2 - c).max())
        print(f"case b {str(dtype)[6:]}: coh^2 against scipy.signal.coherence = {err:.2e}")
        assert err <= 2 * MEASURE_TOL["coh"][i]                                  # d(coh^2) = 2 coh d(coh), coh <= 1


def test_faverage_and_the_chunked_path(isd):
    from isd_amd import connectivity as con
    bands = (("lo", 1.0, 8.0), ("mid", 8.0, 13.0), ("hi", 13.0, 45.0))
    for dtype, _ in DTYPES:
        _, xd = case_data("b", dtype)
        for average in ("segments", "trials"):
            full, f = con.spectral_connectivity(xd, method=["coh", "plv", "imcoh"], average=average, **kw("b"))
            avg, fb = con.spectral_connectivity(xd, method=["coh", "plv", "imcoh"], average=average, faverage=True,
                                                bands=bands, **kw("b"))
            bins = con.band_bins(f, bands)
            assert np.allclose(fb, [f[b].mean() for b in bins])
            for v, a in zip(full, avg):
                assert tuple(a.shape) == tuple(v.shape[:-3]) + (3,) + tuple(v.shape[-2:])
                for k, b in enumerate(bins):
                    want = v[..., int(b[0]):int(b[-1]) + 1, :, :].mean(-3)
                    eps = 1e-6 if dtype == torch.float32 else 1e-14       # the same mean in another order
                    assert torch.allclose(a[..., k, :, :], want, rtol=eps, atol=eps)
        _, xd = case_data("big", dtype)
        args = dict(method=["coh", "ppc"], average="segments", faverage=True, bands=(("all", 2.0, 60.0),), **kw("big"))
        whole = con.spectral_connectivity(xd, **args)[0]
        before = con.CON_CHUNK_BYTES
        try:
            con.CON_CHUNK_BYTES = 7 * 33 * 4 * 4 * 16 * 2                       # 7 trials per chunk
            parts = con.spectral_connectivity(xd, **args)[0]
        finally:
            con.CON_CHUNK_BYTES = before
        for w, p in zip(whole, parts):
            assert tuple(p.shape) == (300, 1, 4, 4) and torch.equal(w, p)


# --------------------------------------------------------------------------------------------------------- CoSpectra
def test_cospectra_on_case_b(isd):
    shape, sfreq = CASES["b"][:2]
    for dtype, tol in DTYPES:
        x, xd = case_data("b", dtype)
        est = isd.riemann.CoSpectra(window=128, overlap=0.75, fmin=4.0, fmax=40.0, fs=sfreq)
        got = est.fit_transform(xd)
        ref, f, _ = ref_csd(x, sfreq, 128, 128, 96, 4.0, 40.0, np.hanning(128))
        K = f.size
        assert tuple(got.shape) == (2, 4, 4, K) and got.dtype == dtype and np.array_equal(est.freqs_, f)
        assert torch.equal(got, got.transpose(1, 2))
        err = float(np.abs(got.cpu().numpy() - ref.real.transpose(0, 2, 3, 1)).max() / np.abs(ref).max())
        print(f"CoSpectra case b {str(dtype)[6:]}: {err:.2e}")
        assert err <= tol
        for k in range(K):
            ts = isd.riemann.TangentSpace().fit_transform(got[..., k].contiguous())
            assert tuple(ts.shape) == (2, 10) and torch.isfinite(ts).all()
    out = isd.riemann.CoSpectra(window=128, fs=sfreq).transform(x)                 # ndarray in -> float64 ndarray
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == (2, 4, 4, 65)


# ---------------------------------------------------------------------------------------------------------- envelope
def test_abi_envelope_and_empty_input(isd):
    from isd_amd import _lib
    L = _lib.lib()
    plan = isd.psd.WelchPlan(64, 64, 32, 0, 32, np.ones(64), 128.0, True)
    x = torch.zeros(2 * 129 * 128, device="cuda")
    out = torch.zeros(2 * 33 * 129 * 129 * 2, device="cuda")
    work = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(n, Cc, T, outp=out.data_ptr()):
        rc = L.isd_csd_welch_f32(plan._h, x.data_ptr(), outp, n, Cc, T, 0, 0, work.data_ptr(), st)
        return rc, L.isd_last_error()

    rc, msg = call(2, 129, 128)
    assert rc == _lib.ISD_ERR_UNSUPPORTED and b"C=129" in msg
    rc, msg = call(2, 4, 63)
    assert rc == _lib.ISD_ERR_UNSUPPORTED and b"shorter than n_per_seg" in msg
    assert call(2, 4, 128, None)[0] == _lib.ISD_ERR_INVALID
    assert call(0, 4, 128)[0] == 0
    torch.cuda.synchronize()
    assert not out.any()                                                           # nothing was launched
    assert L.isd_csd_work_bytes(plan._h, 2, 129, 128, 0, 0) == _lib.ISD_ERR_INVALID
    assert L.isd_csd_work_bytes(plan._h, 2, 4, 128, 1, 1) > 0
    assert L.isd_csd_chunk_bytes(-1) == 256 << 20
    for dtype, _ in DTYPES:
        empty = torch.zeros(0, 4, 795, dtype=dtype, device="cuda")
        got, freqs = isd.connectivity.csd_array_welch(empty, 250)
        assert tuple(got.shape) == (0, 129, 4, 4) and freqs.shape == (129,)
        assert got.dtype == (torch.complex128 if dtype == torch.float64 else torch.complex64)
