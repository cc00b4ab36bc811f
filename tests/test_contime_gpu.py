"""isd_amd.connectivity.spectral_connectivity_time and contime_launch (csrc/contime.hip) on the GPU against the NumPy
float64 restatement of tests/contime_ref.py (itself pinned by hand-computed values in test_contime_cpu.py).

The kernel tests feed the complex map directly: contime_ref.make's complex64 values, widened for the reference, so
the transform's rounding is not in the comparison.  Errors are the largest absolute error of a measure over every
entry.  The diagonal is compared with what the docstring says it holds (contime_ref.DIAGONAL), which the formulas
give to 1e-15 (test_contime_cpu.py); no entry is left out.

Sign-based measures ('pli', 'dpli'): their sums are integers, so with every |Im s| / (|w_i| |w_j|) of the reference
above 1e-6 (asserted first, on the reference alone) the kernel must give the reference's quotient rounded once to the
output's type: EXACT = 1e-12 against that.  'dpli' above the diagonal is stored as 1 - dpli[i, j] in the output's
arithmetic (the bitwise rule), so there the comparison is with that expression of the rounded reference, and with the
independent reference to two roundings of the output type (2 x 2^-24 float32, 2 x 2^-53 float64).

Continuous measures: TOL is 8 x the worst error observed on an MI355X per (group of tests, measure, precision), rounded
up to one digit; the kernel is bitwise repeatable, so the margin covers other library versions of sqrt / divide and a
later reordering of the epilogue only.  An error above DEFECT (1e-4 fp32, 1e-9 fp64) fails whatever TOL says.
Groups: 'cases' (the four cases over their whole length, all eight methods at once, each alone and one pair of every
two groups of sums: every template instance), 'window' (case tiles over four windows, two of them one sample long,
where ciplv = |Im u| / sqrt(1 - (Re u)^2) amplifies the rounding of u without bound as |Re u| -> 1) and 'call' (the
whole call on real data, transform included).

Observed on an MI355X (each test prints its own figures):
  cases  fp64: coh 4.4e-16  imcoh 2.8e-16  plv 3.3e-16  ciplv 2.2e-16  wpli 5.6e-16  wpli2_debiased 1.0e-15
  cases  fp32: coh 4.5e-08  imcoh 4.1e-08  plv 5.3e-08  ciplv 5.3e-08  wpli 4.6e-08  wpli2_debiased 4.5e-08
  window fp64: coh 6.7e-16  imcoh 4.4e-16  plv 5.6e-16  ciplv 1.0e-10  wpli 3.3e-16  wpli2_debiased 2.2e-16
  window fp32: coh 1.2e-07  imcoh 1.4e-07  plv 2.4e-07  ciplv 7.3e-02  wpli 2.4e-08  wpli2_debiased 1.1e-08
  call   fp64: coh 3.3e-16  imcoh 2.5e-16  plv 2.8e-16  ciplv 2.8e-16  wpli 4.4e-16  wpli2_debiased 6.7e-16
  call   fp32: coh 4.8e-08  plv 2.9e-08  wpli 7.4e-08
  pli and dpli: 0 against the rounded reference in every test; at most 4.2e-8 float32 / 1.1e-16 float64 from the
  unrounded one.  float32 ciplv over a one-sample window is 2.7e-3 and 7.3e-2 away (of a true value of 1): the
  conditioning named above, which is why the public function takes ciplv through fp64.
"""

import numpy as np
import pytest
import torch

from contime_ref import (CASES, DEAD, DIAGONAL, METHODS, SIGN_BASED, make, ref_contime, ref_spectral_connectivity_time,
                         sign_margin)

pytestmark = pytest.mark.gpu

PRECISIONS = [(torch.complex128, "fp64"), (torch.complex64, "fp32")]
EXACT = 1e-12
ROUNDING = {"fp32": 2.0 ** -24, "fp64": 2.0 ** -53}
DEFECT = {"fp32": 1e-4, "fp64": 1e-9}
MARGIN = 1e-6
# one pair of measures for every two groups of sums (Hermitian + unit, Hermitian + lag, unit + lag)
GROUP_PAIRS = (("imcoh", "ciplv"), ("coh", "wpli"), ("plv", "wpli2_debiased"))
OBSERVED = {                         # (group, measure, precision) -> worst error observed on an MI355X
    ("cases", "coh", "fp64"): 4.44e-16, ("cases", "imcoh", "fp64"): 2.78e-16, ("cases", "plv", "fp64"): 3.33e-16, ("cases", "ciplv", "fp64"): 2.22e-16, ("cases", "wpli", "fp64"): 5.55e-16, ("cases", "wpli2_debiased", "fp64"): 9.99e-16,
    ("cases", "coh", "fp32"): 4.47e-08, ("cases", "imcoh", "fp32"): 4.12e-08, ("cases", "plv", "fp32"): 5.31e-08, ("cases", "ciplv", "fp32"): 5.27e-08, ("cases", "wpli", "fp32"): 4.65e-08, ("cases", "wpli2_debiased", "fp32"): 4.46e-08,
    ("window", "coh", "fp64"): 6.66e-16, ("window", "imcoh", "fp64"): 4.44e-16, ("window", "plv", "fp64"): 5.55e-16, ("window", "ciplv", "fp64"): 1.03e-10, ("window", "wpli", "fp64"): 3.33e-16, ("window", "wpli2_debiased", "fp64"): 2.22e-16,
    ("window", "coh", "fp32"): 1.19e-07, ("window", "imcoh", "fp32"): 1.39e-07, ("window", "plv", "fp32"): 2.38e-07, ("window", "ciplv", "fp32"): 7.27e-02, ("window", "wpli", "fp32"): 2.44e-08, ("window", "wpli2_debiased", "fp32"): 1.11e-08,
    ("call", "coh", "fp64"): 3.33e-16, ("call", "imcoh", "fp64"): 2.50e-16, ("call", "plv", "fp64"): 2.78e-16, ("call", "ciplv", "fp64"): 2.78e-16, ("call", "wpli", "fp64"): 4.44e-16, ("call", "wpli2_debiased", "fp64"): 6.66e-16,
    ("call", "coh", "fp32"): 4.76e-08, ("call", "plv", "fp32"): 2.88e-08, ("call", "wpli", "fp32"): 7.42e-08,
}
TOL = {                              # 8 x OBSERVED, rounded up to one digit
    ("cases", "coh", "fp64"): 4e-15, ("cases", "imcoh", "fp64"): 3e-15, ("cases", "plv", "fp64"): 3e-15, ("cases", "ciplv", "fp64"): 2e-15, ("cases", "wpli", "fp64"): 5e-15, ("cases", "wpli2_debiased", "fp64"): 8e-15,
    ("cases", "coh", "fp32"): 4e-07, ("cases", "imcoh", "fp32"): 4e-07, ("cases", "plv", "fp32"): 5e-07, ("cases", "ciplv", "fp32"): 5e-07, ("cases", "wpli", "fp32"): 4e-07, ("cases", "wpli2_debiased", "fp32"): 4e-07,
    ("window", "coh", "fp64"): 6e-15, ("window", "imcoh", "fp64"): 4e-15, ("window", "plv", "fp64"): 5e-15, ("window", "ciplv", "fp64"): 9e-10, ("window", "wpli", "fp64"): 3e-15, ("window", "wpli2_debiased", "fp64"): 2e-15,
    ("window", "coh", "fp32"): 1e-06, ("window", "imcoh", "fp32"): 2e-06, ("window", "plv", "fp32"): 2e-06, ("window", "ciplv", "fp32"): 0.6, ("window", "wpli", "fp32"): 2e-07, ("window", "wpli2_debiased", "fp32"): 9e-08,
    ("call", "coh", "fp64"): 3e-15, ("call", "imcoh", "fp64"): 2e-15, ("call", "plv", "fp64"): 3e-15, ("call", "ciplv", "fp64"): 3e-15, ("call", "wpli", "fp64"): 4e-15, ("call", "wpli2_debiased", "fp64"): 6e-15,
    ("call", "coh", "fp32"): 4e-07, ("call", "plv", "fp32"): 3e-07, ("call", "wpli", "fp32"): 6e-07,
}
_CACHE = {}


@pytest.fixture(scope="module")
def con():
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd.connectivity


def case_z(case):
    """-> the complex128 map of a case as the reference sees it (read-only)."""
    if case not in _CACHE:
        z = make(case).astype(np.complex128)
        z.setflags(write=False)
        _CACHE[case] = z
    return _CACHE[case]


def reference(case, t0, t1):
    key = (case, t0, t1)
    if key not in _CACHE:
        z = case_z(case)
        assert sign_margin(z, t0, t1) > MARGIN, (case, t0, t1)
        r = ref_contime(z, METHODS, t0, t1)
        for v in r.values():
            v.setflags(write=False)
        _CACHE[key] = r
    return _CACHE[key]


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def compare(failures, group, what, m, got, ref, prec, defect=None):
    """One measure [..., C, C] (ndarray of the output's dtype) against the float64 reference, every entry."""
    defect = DEFECT[prec] if defect is None else defect
    Cc = ref.shape[-1]
    eye = np.eye(Cc, dtype=bool)
    dg = got[..., eye]
    assert np.array_equal(dg, np.full_like(dg, DIAGONAL[m]), equal_nan=True), (what, m, "diagonal")
    if Cc == 1:
        return 0.0
    off = ~eye
    g64 = got.astype(np.float64)
    if m in SIGN_BASED:
        want = ref.astype(got.dtype)                               # the quotient rounded once to the output's type
        indep = float(np.abs(g64 - ref)[..., off].max())
        if m == "dpli":                                            # above the diagonal: 1 - (the rounded lower entry)
            upper = np.triu(np.ones((Cc, Cc), dtype=bool), 1)
            want = np.where(upper, got.dtype.type(1) - np.swapaxes(want, -1, -2), want)
        err = float(np.abs(g64 - want.astype(np.float64))[..., off].max())
        print(f"{group} {what} {m} {prec}: max |err| = {err:.2e} (rounded reference), {indep:.2e} (reference)")
        if err > EXACT:
            failures.append(f"{what} {m} {prec}: {err:.2e} > {EXACT:g} (sums of +-1 and 1/2 are exact)")
        if indep > 2 * ROUNDING[prec]:                             # the quotient's rounding and that of 1 - it
            failures.append(f"{what} {m} {prec}: {indep:.2e} from the reference, above two roundings")
        return err
    assert np.isfinite(ref[..., off]).all() or group == "window", (what, m)
    assert np.array_equal(np.isnan(g64[..., off]), np.isnan(ref[..., off])), (what, m, "NaN pattern")
    err = float(np.nan_to_num(np.abs(g64 - ref)[..., off]).max())
    print(f"{group} {what} {m} {prec}: max |err| = {err:.2e}")
    if err > defect:
        failures.append(f"{what} {m} {prec}: {err:.2e} is above {defect:g}: a defect, not a tolerance")
    elif err > TOL[(group, m, prec)]:
        failures.append(f"{what} {m} {prec}: {err:.2e} > {TOL[(group, m, prec)]:g}")
    return err


def launch(con, zd, names, t0, t1, **kw):
    """-> {name: tensor [n, F, C, C]} of one contime_launch; names in any order."""
    order = sorted(names, key=METHODS.index)
    out = con.contime_launch(zd, con.contime_mask(order), t0, t1, **kw)
    assert out.shape[0] == len(order)
    return {m: out[i] for i, m in enumerate(order)}


# ------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_matches_the_restatement(con, case):
    n, Cc, F, T = CASES[case]
    ref = reference(case, 0, T)
    failures = []
    for cdtype, prec in PRECISIONS:
        zd = torch.tensor(case_z(case), dtype=cdtype).cuda()
        rdtype = torch.float64 if prec == "fp64" else torch.float32
        calls = [("all", METHODS)] + [(m, (m,)) for m in METHODS] + [("+".join(p), p) for p in GROUP_PAIRS]
        for what, names in calls:
            got = launch(con, zd, names, 0, T)
            for m in names:
                assert got[m].dtype == rdtype and tuple(got[m].shape) == (n, F, Cc, Cc)
                compare(failures, "cases", f"{case} [{what}]", m, got[m].cpu().numpy(), ref[m], prec)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ bitwise properties
@pytest.mark.parametrize("case", ["tiles", "wide"])
def test_bitwise_properties(con, case):
    n, Cc, F, T = CASES[case]
    for cdtype, prec in PRECISIONS:
        zd = torch.tensor(case_z(case), dtype=cdtype).cuda()
        a, b = launch(con, zd, METHODS, 0, T), launch(con, zd, METHODS, 0, T)
        lower = torch.tril(torch.ones(Cc, Cc, dtype=torch.bool, device=zd.device), -1)
        for m in METHODS:
            assert same_bits(a[m], b[m]), (m, prec, "two launches differ")
            v, vt = a[m], a[m].transpose(-1, -2)
            if m == "imcoh":
                assert same_bits(vt[..., lower], -v[..., lower]), (m, prec)
            elif m == "dpli":
                assert same_bits(vt[..., lower], 1 - v[..., lower]), (m, prec)
            else:
                assert same_bits(vt.contiguous(), v), (m, prec)
            dg = torch.diagonal(v, dim1=-2, dim2=-1).cpu().numpy()
            assert np.array_equal(dg, np.full_like(dg, DIAGONAL[m]), equal_nan=True), (m, prec)


def test_a_dead_channel(con):
    """Channel 17 of case tiles (in the ragged second tile) and channel 2 zeroed: their rows and columns hold what the
    docstring says, and every other entry has the bits of the same case with those channels deleted."""
    n, Cc, F, T = CASES["tiles"]
    dead = [2, 17]
    for cdtype, prec in PRECISIONS:
        z = case_z("tiles").copy()
        z[:, dead] = 0
        got = launch(con, torch.tensor(z, dtype=cdtype).cuda(), METHODS, 0, T)
        zl = np.ascontiguousarray(np.delete(z, dead, 1))
        live = launch(con, torch.tensor(zl, dtype=cdtype).cuda().contiguous(), METHODS, 0, T)
        for m in METHODS:
            g = got[m].cpu().numpy()
            for d in dead:
                for line in (np.delete(g[:, :, d, :], d, -1), np.delete(g[:, :, :, d], d, -1)):
                    assert np.array_equal(line, np.full_like(line, DEAD[m]), equal_nan=True), (m, prec, d)
                assert np.array_equal(g[:, :, d, d], np.full_like(g[:, :, d, d], DIAGONAL[m]), equal_nan=True)
            rest = torch.tensor(np.delete(np.delete(g, dead, 2), dead, 3))
            assert same_bits(rest, live[m].cpu()), (m, prec, "a dead channel touched another entry")


# -------------------------------------------------------------------------------------------------------- the window
WINDOWS = ((0, 70), (3, 67), (16, 17), (69, 70))


@pytest.mark.parametrize("t0,t1", WINDOWS)
def test_window(con, t0, t1):
    n, Cc, F, T = CASES["tiles"]
    ref = reference("tiles", t0, t1)
    failures = []
    for cdtype, prec in PRECISIONS:
        z = case_z("tiles")
        zd = torch.tensor(z, dtype=cdtype).cuda()
        got = launch(con, zd, METHODS, t0, t1)
        for m in METHODS:
            defect = None
            if m == "ciplv" and t1 - t0 == 1:
                # one sample: |u| = 1 and ciplv = |Im u| / sqrt(1 - (Re u)^2) = 1; a relative error e of u moves
                # 1 - (Re u)^2 = (Im u)^2 by up to 2 e, the quotient by e / (Im u)^2, and |Im u| is the margin
                defect = 8 * ROUNDING[prec] / sign_margin(case_z("tiles"), t0, t1) ** 2
            compare(failures, "window", f"[{t0}, {t1})", m, got[m].cpu().numpy(), ref[m], prec, defect)
        # a poisoned guard: NaN outside the window changes nothing
        zp = z.copy()
        zp[..., :t0] = np.nan
        zp[..., t1:] = np.nan
        poisoned = launch(con, torch.tensor(zp, dtype=cdtype).cuda(), METHODS, t0, t1)
        for m in METHODS:
            assert same_bits(poisoned[m], got[m]), (m, prec, "samples outside [t0, t1) were read")
        # out= as a view into a larger NaN-filled buffer: the surroundings stay NaN
        rdtype = torch.float64 if prec == "fp64" else torch.float32
        numel, pad = len(METHODS) * n * F * Cc * Cc, 1000
        buf = torch.full((numel + 2 * pad,), float("nan"), dtype=rdtype, device=zd.device)
        view = buf[pad:pad + numel].view(len(METHODS), n, F, Cc, Cc)
        ret = con.contime_launch(zd, con.contime_mask(METHODS), t0, t1, out=view)
        assert ret.data_ptr() == view.data_ptr()
        assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + numel:]).all()
        for i, m in enumerate(METHODS):
            assert same_bits(view[i], got[m]), (m, prec)
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------------- the whole call
CALL = dict(freqs=[8.0, 12.0, 20.0], sfreq=100.0, n_cycles=3.0, decim=2, padding=0.1)


def call_data():
    if "call" not in _CACHE:
        x = np.random.default_rng(5).standard_normal((3, 5, 200))
        r, z, t0, t1 = ref_spectral_connectivity_time(x, CALL["freqs"], METHODS, CALL["sfreq"], CALL["n_cycles"],
                                                      CALL["decim"], True, CALL["padding"])
        assert (t0, t1) == (5, 95) and z.shape == (3, 5, 3, 100)
        assert sign_margin(z, t0, t1) > MARGIN
        _CACHE["call"] = (x, r)
    return _CACHE["call"]


def test_whole_call_fp64(con):
    x, ref = call_data()
    failures = []
    got, freqs = con.spectral_connectivity_time(x, method=list(METHODS), **CALL)
    assert np.array_equal(freqs, np.array(CALL["freqs"])) and len(got) == len(METHODS)
    for m, g in zip(METHODS, got):
        assert isinstance(g, np.ndarray) and g.dtype == np.float64 and g.shape == (3, 3, 5, 5)
        compare(failures, "call", "ndarray", m, g, ref[m], "fp64")
    one, _ = con.spectral_connectivity_time(x, method="wpli", **CALL)
    assert isinstance(one, np.ndarray) and np.array_equal(one, got[METHODS.index("wpli")], equal_nan=True)
    # [C, T] is n = 1
    single, _ = con.spectral_connectivity_time(x[1], method="coh", **CALL)
    assert single.shape == (1, 3, 5, 5) and np.abs(single - got[0][1:2])[..., ~np.eye(5, dtype=bool)].max() <= 1e-12
    # average=True: the mean of the per-trial result (fp64 sums in trial order; 3 trials: within a few roundings)
    avg, _ = con.spectral_connectivity_time(x, method=list(METHODS), average=True, **CALL)
    for m, a, g in zip(METHODS, avg, got):
        assert a.shape == (3, 5, 5)
        assert np.array_equal(np.isnan(a), np.isnan(g.mean(0))), m
        err = float(np.nan_to_num(np.abs(a - g.mean(0))).max())
        print(f"average {m}: max |err| = {err:.2e}")
        assert err <= 4 * 2.0 ** -52, m
    # faverage=True with two bands: the mean over each band's frequencies
    bands = [("low", 7.0, 13.0), ("beta", 15.0, 25.0)]
    fav, bf = con.spectral_connectivity_time(x, method=["coh", "dpli"], faverage=True, bands=bands, **CALL)
    assert np.allclose(bf, [10.0, 20.0], rtol=0, atol=1e-12)
    for m, v in zip(("coh", "dpli"), fav):
        g = got[METHODS.index(m)]
        want = np.stack([g[:, :2].mean(1), g[:, 2:].mean(1)], axis=1)
        assert v.shape == (3, 2, 5, 5) and np.abs(v - want).max() <= 4 * 2.0 ** -52, m
    assert not failures, "\n".join(failures)


def test_whole_call_fp32_and_chunks(con, monkeypatch):
    x, ref = call_data()
    failures = []
    xd = torch.tensor(x, dtype=torch.float32).cuda()
    names = ["coh", "plv", "wpli"]
    got, _ = con.spectral_connectivity_time(xd, method=names, **CALL)
    for m, g in zip(names, got):
        assert g.is_cuda and g.dtype == torch.float32 and tuple(g.shape) == (3, 3, 5, 5)
        compare(failures, "call", "float32 tensor", m, g.cpu().numpy(), ref[m], "fp32")
    # three chunks of one trial give the bits of one chunk
    per_trial = 5 * 3 * 100 * 8
    monkeypatch.setattr(con, "CONTIME_CHUNK_BYTES", per_trial + 1)
    chunked, _ = con.spectral_connectivity_time(xd, method=names, **CALL)
    for m, a, b in zip(names, chunked, got):
        assert same_bits(a, b), (m, "chunked")
    x64 = torch.tensor(x).cuda()
    monkeypatch.setattr(con, "CONTIME_CHUNK_BYTES", 256 << 20)
    whole, _ = con.spectral_connectivity_time(x64, method=list(METHODS), **CALL)
    monkeypatch.setattr(con, "CONTIME_CHUNK_BYTES", 2 * per_trial + 1)
    chunked, _ = con.spectral_connectivity_time(x64, method=list(METHODS), **CALL)
    for m, a, b in zip(METHODS, chunked, whole):
        assert a.dtype == torch.float64 and same_bits(a, b), (m, "chunked fp64")
    monkeypatch.setattr(con, "CONTIME_CHUNK_BYTES", 256 << 20)
    # ciplv on a float32 tensor: the fp64 route, rounded at the end
    (ci, pl), _ = con.spectral_connectivity_time(xd, method=["ciplv", "plv"], **CALL)
    off = ~np.eye(5, dtype=bool)
    for m, v in (("ciplv", ci), ("plv", pl)):
        assert v.dtype == torch.float32
        # float32 data, so the reference is that of the rounded data
        r32 = ref_spectral_connectivity_time(x.astype(np.float32).astype(np.float64), CALL["freqs"], (m,),
                                             CALL["sfreq"], CALL["n_cycles"], CALL["decim"], True,
                                             CALL["padding"])[0][m]
        err = float(np.abs(v.cpu().numpy().astype(np.float64) - r32)[..., off].max())
        print(f"call float32 tensor with ciplv {m}: max |err| = {err:.2e}")
        assert err <= 2.0 ** -24 + TOL[("call", m, "fp64")], m      # one rounding of a result <= 1 to float32
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------------------ the ABI
def test_abi_errors_launch_nothing(con):
    from isd_amd import _lib
    L = _lib.lib()
    n, Cc, F, T = 1, 4, 2, 8
    z = torch.zeros(n, 129, F, T, 2, device="cuda")
    out = torch.full((8 * n * F * 129 * 129,), float("nan"), device="cuda")
    st = _lib.stream()

    def call(C_, t0, t1, mask, average=0, n_=n):
        return L.isd_contime_f32(z.data_ptr(), out.data_ptr(), n_, C_, F, T, t0, t1, mask, average, st)
    assert call(129, 0, T, 1) == _lib.ISD_ERR_UNSUPPORTED
    assert call(0, 0, T, 1) == _lib.ISD_ERR_UNSUPPORTED
    for t0, t1 in ((4, 4), (5, 3), (-1, 4), (0, T + 1)):
        assert call(Cc, t0, t1, 1) == _lib.ISD_ERR_INVALID
    assert call(Cc, 0, T, 0) == _lib.ISD_ERR_INVALID               # an empty mask
    assert call(Cc, 0, T, 256) == _lib.ISD_ERR_INVALID
    assert call(Cc, 0, T, 1, n_=-1) == _lib.ISD_ERR_INVALID
    assert call(Cc, 0, T, 1, average=1, n_=0) == _lib.ISD_ERR_INVALID
    assert L.isd_contime_f32(None, out.data_ptr(), n, Cc, F, T, 0, T, 1, 0, st) == _lib.ISD_ERR_INVALID
    assert call(Cc, 0, T, 1, n_=0) == _lib.ISD_OK
    assert b"isd_contime_f32" in L.isd_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "an invalid call wrote to out"
    with pytest.raises(ValueError, match="out must be"):
        con.contime_launch(torch.zeros(1, 4, 2, 8, dtype=torch.complex64, device="cuda"), 3, 0, 8,
                           out=torch.zeros(1, 1, 2, 4, 4, device="cuda"))
