"""isd_amd.connectivity.envelope_correlation, isd_amd.hilbert and isd_amd.envelope on the GPU against the NumPy float64
restatement of tests/envelope_ref.py (itself pinned by scipy.signal.hilbert and np.corrcoef in test_envelope_cpu.py).

The kernel tests feed complex z directly: scipy.signal.hilbert of envelope_ref.make's data, rounded to the tested
precision and widened again for the reference, so the FFT's rounding is not in the comparison.  Errors are the largest
absolute error of a correlation.  NaN entries of a log reference would be excluded, and the case data has none
(asserted on the reference): the log variants leave out t1 and t2, whose z is real (o = 0, log o = -inf).

Bounds: TOL is 8 x the worst error observed on an MI355X per (precision, variant), rounded up to one digit -- the
kernels are bitwise repeatable, so the margin covers other clocks and library versions of the elementwise steps only.
An error above DEFECT (1e-10 fp64, 1e-4 fp32; 1e-6 for fp32 with log=True) is a defect, not a tolerance, and fails
whatever TOL says: the issue's emulation in fp32 arithmetic puts an uncompensated cross product a_l b_j - b_l a_j at
8.0e-6 / 3.1e-6 on cases b and c with log=True and Kahan's compensated form at 1.6e-8 / 7.8e-9.

Observed on an MI355X (worst over the cases, the dead-channel and the scale test and over absolute on / off; each test
prints its own figures):
  pairwise       2.1e-15 fp64 (c)     3.4e-8 fp32 (c128)       pairwise, log   1.8e-14 fp64 (c)     5.0e-8 fp32 (c128)
  plain          1.3e-15 fp64 (b)     1.2e-7 fp32 (t2: +-1 rounded to float32)
  plain, log     1.6e-15 fp64 (big)   3.6e-8 fp32 (c128)
  case b x 1e-6  pairwise 3.9e-16 / 1.7e-8, log 1.4e-15 / 1.5e-8, plain 1.3e-15 / 1.8e-8, plain log 1.1e-15 / 1.6e-8
  hilbert, envelope over the largest |reference|:  1.3e-15 fp64 (T = 795, N = 824),  3.7e-7 fp32 (T = 64, N = 93)

The scale test feeds case b times 1e-6 (volts), rounded to the tested precision, and compares with the restatement of
that rounded input times 1e6, i.e. at the unscaled size: rounding z x 1e-6 to float32 afresh would move the cross
product of two nearly in-phase channels by as much as an uncompensated product does, which is the input's doing and
not the kernel's.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.signal as ss
import torch

from envelope_ref import CASES, make, ref_envcorr
from test_envelope_cpu import LENGTHS, lengths_of

pytestmark = pytest.mark.gpu

PRECISIONS = [(torch.complex128, "fp64"), (torch.complex64, "fp32")]
# variant -> (orthogonalize, log); each is run with absolute on and off where it matters
VARIANTS = {"pairwise": ("pairwise", False), "pairwise_log": ("pairwise", True), "plain": (False, False),
            "plain_log": (False, True)}
DEFECT = {("fp64", False): 1e-10, ("fp64", True): 1e-10, ("fp32", False): 1e-4, ("fp32", True): 1e-6}
OBSERVED = {                         # (precision, variant) -> worst error observed on an MI355X
    ("fp64", "pairwise"): 2.05e-15, ("fp64", "pairwise_log"): 1.76e-14, ("fp64", "plain"): 1.33e-15,
    ("fp64", "plain_log"): 1.55e-15, ("fp32", "pairwise"): 3.40e-8, ("fp32", "pairwise_log"): 5.01e-8,
    ("fp32", "plain"): 1.19e-7, ("fp32", "plain_log"): 3.59e-8,
}
TOL = {                              # 8 x OBSERVED, rounded up to one digit
    ("fp64", "pairwise"): 2e-14, ("fp64", "pairwise_log"): 2e-13, ("fp64", "plain"): 2e-14,
    ("fp64", "plain_log"): 2e-14, ("fp32", "pairwise"): 3e-7, ("fp32", "pairwise_log"): 5e-7,
    ("fp32", "plain"): 1e-6, ("fp32", "plain_log"): 3e-7,
}
HILBERT_OBSERVED = {"fp64": 1.28e-15, "fp32": 3.71e-7}
HILBERT_TOL = {"fp64": 2e-14, "fp32": 3e-6}      # 8 x HILBERT_OBSERVED, rounded up to one digit
REAL_CASES = ("t2",)                 # cases fed real-valued z
NO_LOG = ("t1", "t2")                # real z: log o = -inf
_CACHE = {}


@pytest.fixture(scope="module")
def isd():
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd


def shape_of(case):
    if case == "long":
        from isd_amd.connectivity import ENVCORR_CHUNK
        return (1, 4, 3 * ENVCORR_CHUNK + 7)
    return CASES[case]


ALL_CASES = sorted(CASES) + ["long"]


def case_z(case, cdtype, scale=1.0):
    """-> (z as the reference sees it, complex128 ndarray, read-only; z on the device in cdtype)."""
    key = ("z", case, cdtype, scale)
    if key not in _CACHE:
        x = make(*shape_of(case), seed=sorted(ALL_CASES).index(case) + 11)
        z = x.astype(np.complex128) if case in REAL_CASES else ss.hilbert(x, axis=-1)
        z = z * scale
        if cdtype == torch.complex64:
            z = z.astype(np.complex64).astype(np.complex128)
        z.setflags(write=False)
        _CACHE[key] = z
    z = _CACHE[key]
    return z, torch.tensor(z, dtype=cdtype).cuda()


def reference(case, cdtype, orth, log, absolute):
    key = ("ref", case, cdtype, orth, log, absolute)
    if key not in _CACHE:
        r = ref_envcorr(case_z(case, cdtype)[0], orth, log, absolute)
        assert not np.isnan(r).any(), (case, orth, log)
        r.setflags(write=False)
        _CACHE[key] = r
    return _CACHE[key]


def check(failures, what, err, prec, variant):
    log = VARIANTS[variant][1]
    if err > DEFECT[(prec, log)]:
        failures.append(f"{what}: {err:.2e} is above {DEFECT[(prec, log)]:g}: a defect, not a tolerance")
    elif err > TOL[(prec, variant)]:
        failures.append(f"{what}: {err:.2e} > {TOL[(prec, variant)]:g}")


# ------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("case,variant", [(c, v) for c in ALL_CASES for v in sorted(VARIANTS)
                                          if not (VARIANTS[v][1] and c in NO_LOG)])
def test_matches_the_restatement(isd, case, variant):
    orth, log = VARIANTS[variant]
    failures = []
    for cdtype, prec in PRECISIONS:
        _, zd = case_z(case, cdtype)
        for absolute in ((True, False) if orth else (True,)):
            ref = reference(case, cdtype, orth, log, absolute)
            got = isd.connectivity.envelope_correlation(zd, orthogonalize=orth, log=log, absolute=absolute)
            assert got.is_cuda and got.dtype == (torch.float64 if prec == "fp64" else torch.float32)
            assert tuple(got.shape) == ref.shape
            err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
            print(f"case {case} {variant} absolute={absolute} {prec}: max |err| = {err:.2e}")
            check(failures, f"{prec} absolute={absolute}", err, prec, variant)
            # structure
            dg = torch.diagonal(got, dim1=-2, dim2=-1).cpu().numpy()
            assert torch.equal(got, got.transpose(-1, -2))
            if orth:
                assert (dg == 0).all()
            else:                                                      # exactly 1, or 0 for a row of zero norm (T = 1)
                assert np.array_equal(dg, np.rint(np.diagonal(ref, axis1=-2, axis2=-1)))
    assert not failures, failures


def test_degenerate_cases_are_finite_and_the_restatement(isd):
    failures = []
    for cdtype, prec in PRECISIONS:
        for case in ("t1", "t2", "c1"):
            _, zd = case_z(case, cdtype)
            for variant in ("pairwise", "plain"):
                orth = VARIANTS[variant][0]
                for absolute in (True, False):
                    got = isd.connectivity.envelope_correlation(zd, orthogonalize=orth, absolute=absolute)
                    assert torch.isfinite(got).all()
                    ref = reference(case, cdtype, orth, False, absolute)
                    if orth or case == "t1":
                        assert not ref.any() and not got.any(), (case, variant)      # exact zeros
                    err = float(np.abs(got.cpu().numpy() - ref).max())
                    check(failures, f"{case} {variant} {prec}", err, prec, variant)
        z, zd = case_z("a", cdtype)
        z, zd = z.copy(), zd.clone()
        z[:, 2] = 0
        zd[:, 2] = 0
        for variant in ("pairwise", "plain"):
            orth = VARIANTS[variant][0]
            got = isd.connectivity.envelope_correlation(zd, orthogonalize=orth)
            assert torch.isfinite(got).all() and not got[:, 2].any() and not got[:, :, 2].any()
            err = float(np.abs(got.cpu().numpy() - ref_envcorr(z, orth)).max())
            print(f"case a with a dead channel, {variant} {prec}: {err:.2e}")
            check(failures, f"dead channel {variant} {prec}", err, prec, variant)
        got = isd.connectivity.envelope_correlation(zd, log=True).cpu().numpy()         # NaN where the zero enters only
        ref = ref_envcorr(z, log=True)
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        ok = ~np.isnan(ref)
        check(failures, f"dead channel pairwise_log {prec}", float(np.abs(got - ref)[ok].max()), prec, "pairwise_log")
    assert not failures, failures


def test_microvolt_scale(isd):
    failures = []
    for cdtype, prec in PRECISIONS:
        zs, zd = case_z("b", cdtype, 1e-6)
        for variant, (orth, log) in sorted(VARIANTS.items()):
            ref = ref_envcorr(zs * 1e6, orth, log)
            assert not np.isnan(ref).any()
            got = isd.connectivity.envelope_correlation(zd, orthogonalize=orth, log=log)
            err = float(np.abs(got.cpu().numpy() - ref).max())
            print(f"case b x 1e-6 {variant} {prec}: max |err| = {err:.2e}")
            check(failures, f"{variant} {prec}", err, prec, variant)
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------- the kernel
def fenced(shape, dtype, shift):
    """A contiguous view of `shape` inside a larger NaN-filled device buffer, `shift` elements off its start."""
    pad, size = 64, int(np.prod(shape))
    nan = complex("nan+nanj") if dtype.is_complex else float("nan")
    buf = torch.full((size + 2 * pad + shift,), nan, dtype=dtype, device="cuda")
    return buf, buf[pad + shift:pad + shift + size].view(shape)


@pytest.mark.parametrize("case", ["a", "c", "c128", "big", "long"])
def test_nan_fences_around_z_and_out_stay_intact(isd, case):
    from isd_amd import connectivity as con
    for cdtype, prec in PRECISIONS:
        _, zd = case_z(case, cdtype)
        n, Cc, T = zd.shape
        rdtype = torch.float64 if prec == "fp64" else torch.float32
        for flags in (con.ENV_ABSOLUTE, con.ENV_ABSOLUTE | con.ENV_LOG, con.ENV_PLAIN, con.ENV_PLAIN | con.ENV_LOG):
            clean = con.envcorr_launch(zd, flags)
            for shift in (1, 3):
                zbuf, zv = fenced(tuple(zd.shape), cdtype, shift)
                zv.copy_(zd)
                obuf, ov = fenced((n, Cc, Cc), rdtype, shift)
                got = con.envcorr_launch(zv, flags, out=ov)
                assert got.data_ptr() == ov.data_ptr()
                assert torch.isfinite(got).all() and torch.equal(got, clean)
                for buf in (torch.view_as_real(zbuf), obuf):
                    assert torch.isnan(buf[:64]).all() and torch.isnan(buf[-64:]).all(), (prec, flags, shift)


def test_two_calls_and_views_give_the_same_bits(isd):
    con = isd.connectivity
    for cdtype, prec in PRECISIONS:
        for case in ("a", "c", "big"):
            _, zd = case_z(case, cdtype)
            for kw in (dict(), dict(log=True), dict(orthogonalize=False), dict(absolute=False)):
                assert torch.equal(con.envelope_correlation(zd, **kw), con.envelope_correlation(zd, **kw)), (case, kw)
        _, zd = case_z("a", cdtype)
        wide = torch.zeros(3, 5, 2 * 65, dtype=cdtype, device="cuda")
        wide[..., ::2] = zd
        view = wide[..., ::2]
        assert not view.is_contiguous()
        assert torch.equal(con.envelope_correlation(view), con.envelope_correlation(zd))
        one = con.envelope_correlation(zd[1])                                    # [C, T] is n = 1
        assert tuple(one.shape) == (5, 5) and torch.equal(one, con.envelope_correlation(zd)[1])


def test_routes(isd):
    con = isd.connectivity
    z, zd = case_z("b", torch.complex128)
    for kw in (dict(), dict(log=True, absolute=False), dict(orthogonalize=False)):
        got = con.envelope_correlation(np.array(z), **kw)                        # complex ndarray: the fp64 route
        assert isinstance(got, np.ndarray) and got.dtype == np.float64
        assert np.array_equal(got, con.envelope_correlation(zd, **kw).cpu().numpy())
    x = make(*CASES["b"], seed=3)
    for dtype in (torch.float64, torch.float32):
        xd = torch.tensor(x, dtype=dtype).cuda()
        for kw in (dict(), dict(log=True), dict(orthogonalize=False)):
            real = con.envelope_correlation(xd, **kw)                            # real input goes through hilbert
            assert real.dtype == dtype and torch.equal(real, con.envelope_correlation(isd.hilbert(xd), **kw))
    got = con.envelope_correlation(x.astype(np.float32))                         # real ndarray: fp64 too
    assert got.dtype == np.float64
    assert np.array_equal(got, con.envelope_correlation(torch.tensor(x.astype(np.float32)).double().cuda()).cpu().numpy())
    err = float(np.abs(con.envelope_correlation(x) - ref_envcorr(ss.hilbert(x, axis=-1))).max())
    print(f"real case b through hilbert, fp64: {err:.2e}")
    assert err <= TOL[("fp64", "pairwise")]
    for cdtype, prec in PRECISIONS:
        empty = torch.zeros(0, 4, 16, dtype=cdtype, device="cuda")
        got = con.envelope_correlation(empty)
        assert tuple(got.shape) == (0, 4, 4) and got.dtype == (torch.float64 if prec == "fp64" else torch.float32)


# --------------------------------------------------------------------------------------------- hilbert and envelope
@pytest.mark.parametrize("T,N", [(T, N) for T in LENGTHS for N in lengths_of(T)])
def test_hilbert_and_envelope_are_scipy(isd, T, N):
    """One transform length per case: the FFT library builds its kernels for a new length on first use, which is
    most of a case's time."""
    x = make(2, 3, T, 7)
    failures = []
    for dtype, prec in ((torch.float64, "fp64"), (torch.float32, "fp32")):
        xr = x if prec == "fp64" else x.astype(np.float32).astype(np.float64)
        xd = torch.tensor(xr, dtype=dtype).cuda()
        want = ss.hilbert(xr, N, axis=-1)
        got = isd.hilbert(xd, N)
        assert got.is_cuda and got.dtype == (torch.complex128 if prec == "fp64" else torch.complex64)
        assert tuple(got.shape) == (2, 3, T if N is None else N)
        env = isd.envelope(xd, N)
        assert env.dtype == dtype and tuple(env.shape) == (2, 3, min(T, T if N is None else N))
        scale = np.abs(want).max()
        err = float(np.abs(got.cpu().numpy() - want).max() / scale)
        eerr = float(np.abs(env.cpu().numpy() - np.abs(want)[..., :T]).max() / scale)
        print(f"T={T} N={N} {prec}: hilbert {err:.2e}  envelope {eerr:.2e}")
        for what, e in (("hilbert", err), ("envelope", eerr)):
            line = 1e-10 if prec == "fp64" else 1e-4
            if e > line:
                failures.append(f"{what} T={T} N={N} {prec}: {e:.2e} is above {line:g}: a defect")
            elif e > HILBERT_TOL[prec]:
                failures.append(f"{what} T={T} N={N} {prec}: {e:.2e} > {HILBERT_TOL[prec]:g}")
    got = isd.hilbert(x, N)                                                      # ndarray in: fp64, complex128 out
    assert isinstance(got, np.ndarray) and got.dtype == np.complex128
    assert np.array_equal(got, isd.hilbert(torch.tensor(x).cuda(), N).cpu().numpy())
    env = isd.envelope(x.astype(np.float32), N)
    assert isinstance(env, np.ndarray) and env.dtype == np.float64 and env.shape == (2, 3, min(T, N or T))
    assert not failures, failures


# --------------------------------------------------------------------------------------------------------------- ABI
def test_abi_envelope(isd):
    from isd_amd import _lib
    L = _lib.lib()
    z = torch.zeros(2 * 129 * 16 * 2, device="cuda")
    out = torch.full((2 * 129 * 129,), float("nan"), device="cuda")
    nbytes = L.isd_envcorr_work_bytes(2, 128, 16, 0)
    assert nbytes > 0 and L.isd_envcorr_work_bytes(0, 4, 16, 1) > 0
    assert L.isd_envcorr_work_bytes(2, 129, 16, 0) == _lib.ISD_ERR_INVALID
    work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(n, Cc, T, flags=2, workp=work.data_ptr()):
        rc = L.isd_envcorr_f32(z.data_ptr(), out.data_ptr(), n, Cc, T, flags, workp, st)
        return rc, L.isd_last_error()

    assert call(0, 4, 16)[0] == _lib.ISD_OK
    rc, msg = call(2, 129, 16)
    assert rc == _lib.ISD_ERR_UNSUPPORTED and b"C=129" in msg
    rc, msg = call(2, 4, 16, workp=None)
    assert rc == _lib.ISD_ERR_INVALID and b"null" in msg
    rc, msg = call(2, 4, 0)
    assert rc == _lib.ISD_ERR_INVALID and b"T=0" in msg
    assert call(2, 4, 16, flags=8)[0] == _lib.ISD_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                                # nothing was launched
