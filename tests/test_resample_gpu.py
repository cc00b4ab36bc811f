"""isd_amd.resample_poly / resample / Resampler on the GPU against scipy.signal.resample_poly run in float64 (for
float32 input: on the float32 data widened to float64 -- scipy's own float32 path rounds its taps).

Error: max|got − ref| / max|ref| <= 1e-12 (fp64) and 1e-5 (fp32), the bounds of tests/test_fir_gpu.py: an output here
has at most 82 terms with Σ|h| <= 2.25 per phase against the 413 of that product.  Shapes are the smallest that reach
each path: row counts 1 / 15 / 17 / 33 (a 16-row tile short, full plus one, and [3, 11, T] straddling a trial), T = 795
(n_out no multiple of 16, several blocks), 37 and 5 (rows shorter than the filter's half length: 'reflect' folds many
times), 2, and 1 for the pad types scipy survives there; 70 001 rows for the grid.

scipy dies with a floating point exception for a one-sample row with a non-constant upfirdn mode: no case here hands
it one (those go to the NumPy restatement of tests/resample_ref.py)."""
import functools

import numpy as np
import pytest
import torch
from scipy import signal

import resample_ref
from resample_ref import rel_err

pytestmark = pytest.mark.gpu

TOL = {torch.float64: 1e-12, torch.float32: 1e-5}
DTYPES = [torch.float64, torch.float32]


@pytest.fixture(scope="module")
def isd():
    import isd_amd
    return isd_amd


@functools.lru_cache(maxsize=None)
def rows_of(rows, T):
    x = resample_ref.make_rows(rows, T)
    x.setflags(write=False)
    return x


def as_input(x, dtype):
    """-> (CUDA tensor of ``dtype``, the float64 array scipy sees: the rounded data widened)."""
    t = torch.tensor(x, dtype=dtype)
    return t.cuda(), t.double().numpy()


def check(got, ref, dtype, what):
    assert got.dtype == dtype and tuple(got.shape) == ref.shape, what
    err = rel_err(got.cpu().numpy(), ref)
    print(f"{what} {str(dtype)[6:]}: {err:.2e}")
    assert err <= TOL[dtype], what
    return err


@pytest.mark.parametrize("up,down", resample_ref.RATIOS)
def test_ratios_and_shapes(isd, up, down):
    for T in (795, 37, 5, 2):
        for rows in (1, 15, 17, 33):
            x = rows_of(rows, T).reshape((3, 11, T) if rows == 33 else (rows, T))
            for dtype in DTYPES:
                xd, xw = as_input(x, dtype)
                for padtype in ("constant", "reflect"):
                    ref = signal.resample_poly(xw, up, down, axis=-1, padtype=padtype)
                    check(isd.resample_poly(xd, up, down, padtype=padtype), ref, dtype,
                          f"{up}/{down} rows={rows} T={T} {padtype}")


@pytest.mark.parametrize("padtype", resample_ref.PADTYPES)
def test_pad_types_on_offset_rows(isd, padtype):
    """Rows with offsets 0 / 50 / −200; 'mean' in fp32 stays inside the fp32 bound because the offset is taken off in
    fp64 before the data is rounded to the kernel's type."""
    for up, down, T in ((1, 4, 795), (3, 2, 37), (125, 512, 600), (2, 3, 5), (7, 1, 2)):
        for dtype in DTYPES:
            xd, xw = as_input(rows_of(17, T), dtype)
            ref = signal.resample_poly(xw, up, down, axis=-1, padtype=padtype)
            check(isd.resample_poly(xd, up, down, padtype=padtype), ref, dtype, f"{padtype} {up}/{down} T={T}")
            if padtype == "constant":
                ref = signal.resample_poly(xw, up, down, axis=-1, padtype=padtype, cval=2.5)
                check(isd.resample_poly(xd, up, down, padtype=padtype, cval=2.5), ref, dtype, f"cval {up}/{down} T={T}")


def test_one_sample_rows(isd):
    x = rows_of(17, 1)
    for up, down in ((1, 2), (7, 1), (3, 2), (125, 512)):
        for dtype in DTYPES:
            xd, xw = as_input(x, dtype)
            for padtype in ("constant", "mean"):
                ref = signal.resample_poly(xw, up, down, axis=-1, padtype=padtype)
                check(isd.resample_poly(xd, up, down, padtype=padtype), ref, dtype, f"T=1 {padtype} {up}/{down}")
            for padtype in ("edge", "symmetric"):                  # scipy cannot be asked: the restatement
                ref = resample_ref.resample_poly(xw, up, down, padtype=padtype)
                check(isd.resample_poly(xd, up, down, padtype=padtype), ref, dtype, f"T=1 {padtype} {up}/{down}")
            for padtype in ("reflect", "line"):
                with pytest.raises(ValueError, match="two samples"):
                    isd.resample_poly(xd, up, down, padtype=padtype)


@pytest.mark.parametrize("up,down,T", [(1, 1024, 3000), (1024, 1, 5), (1023, 1024, 50), (1024, 1023, 37)])
def test_corners_of_the_envelope(isd, up, down, T):
    """The largest rates: 20 481 taps, a window of 35 844 samples per block at 1/1024, 1023 phase tables at
    1023/1024.  An output has n = ceil(20 481 / up) terms here, up to 20 481 against the 82 the module's bounds were
    set for, so the bound is the larger of those and the rounding of a chained sum of n terms that err independently:
    sqrt(n) u Σ|h| with Σ|h| <= 2.25 and u = 2^-24 / 2^-53 -- 1.9e-5 in fp32 at up = 1, the module's bound otherwise."""
    n_terms = -(-20481 // up)
    for dtype in DTYPES:
        tol = max(TOL[dtype], 2.25 * np.sqrt(n_terms) * (2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53))
        xd, xw = as_input(rows_of(17, T), dtype)
        for padtype in ("constant", "reflect"):
            ref = signal.resample_poly(xw, up, down, axis=-1, padtype=padtype)
            got = isd.resample_poly(xd, up, down, padtype=padtype)
            err = rel_err(got.cpu().numpy(), ref)
            print(f"{up}/{down} T={T} {padtype} {str(dtype)[6:]}: {err:.2e} (bound {tol:.1e})")
            assert got.dtype == dtype and tuple(got.shape) == ref.shape and err <= tol


@pytest.mark.parametrize("n_taps", sorted(resample_ref.TAPS))
def test_explicit_taps(isd, n_taps):
    taps = resample_ref.TAPS[n_taps]
    for up, down, T in ((1, 2, 795), (3, 2, 37), (2, 3, 5), (7, 1, 37), (160, 147, 100)):
        for dtype in DTYPES:
            xd, xw = as_input(rows_of(17, T), dtype)
            for window in (taps, list(taps)):
                for padtype in ("constant", "symmetric"):
                    ref = signal.resample_poly(xw, up, down, axis=-1, window=window, padtype=padtype)
                    check(isd.resample_poly(xd, up, down, window=window, padtype=padtype), ref, dtype,
                          f"{n_taps} taps {up}/{down} T={T} {padtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_rows_than_a_grid_dimension(isd, dtype):
    rows, T = 70001, 9
    x = np.random.default_rng(5).standard_normal((rows, T)) + np.arange(rows)[:, None] % 7
    xd, xw = as_input(x, dtype)
    ref = signal.resample_poly(xw, 1, 2, axis=-1, padtype="edge")
    got = isd.resample_poly(xd, 1, 2, padtype="edge").cpu().numpy().astype(np.float64)
    per_row = np.max(np.abs(got - ref), axis=1) / np.max(np.abs(ref))
    assert got.shape == ref.shape and float(per_row.max()) <= TOL[dtype], int(per_row.argmax())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("padtype", ["constant", "reflect", "mean"])
def test_rows_are_independent(isd, dtype, padtype):
    for up, down, T in ((1, 4, 795), (125, 512, 37)):
        xd, _ = as_input(rows_of(17, T), dtype)
        clean = isd.resample_poly(xd, up, down, padtype=padtype)
        bad = xd.clone()
        bad[3] = float("nan")
        bad[9] = float("inf")
        got = isd.resample_poly(bad, up, down, padtype=padtype)
        keep = [r for r in range(17) if r not in (3, 9)]
        assert torch.equal(got[keep], clean[keep])
        assert not torch.isfinite(got[3]).any()
        for r in (0, 16):                                          # a row alone against the same row in the batch
            assert torch.equal(isd.resample_poly(xd[r:r + 1], up, down, padtype=padtype)[0], clean[r])
        assert torch.equal(isd.resample_poly(xd[5], up, down, padtype=padtype), clean[5])          # [T] in, [n_out] out


@pytest.mark.parametrize("dtype", DTYPES)
def test_repeatable_and_views(isd, dtype):
    xd, xw = as_input(rows_of(33, 795).reshape(3, 11, 795), dtype)
    a = isd.resample_poly(xd, 125, 512, padtype="line")
    b = isd.resample_poly(xd, 125, 512, padtype="line")
    assert torch.equal(a, b)
    view = xd[:, ::2, 1::3]
    assert not view.is_contiguous()
    assert torch.equal(isd.resample_poly(view, 3, 2), isd.resample_poly(view.contiguous(), 3, 2))
    check(isd.resample_poly(view, 3, 2), signal.resample_poly(xw[:, ::2, 1::3], 3, 2, axis=-1), dtype, "view 3/2")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shift", [0, 1])
def test_fences_stay_intact(isd, dtype, shift):
    """NaN fences before and after x and y at element shifts 0 and 1: nothing outside y is written, and a read
    outside x would reach the result."""
    rows, T, fence = 17, 37, 64
    plan = isd.Resampler(3, 2)
    n_out = plan.out_len(T)
    x, xw = as_input(rows_of(rows, T), dtype)
    xbuf = torch.full((rows * T + 2 * fence + 1,), float("nan"), dtype=dtype, device="cuda")
    ybuf = torch.full((rows * n_out + 2 * fence + 1,), float("nan"), dtype=dtype, device="cuda")
    xs = xbuf[fence + shift:fence + shift + rows * T].view(rows, T)
    ys = ybuf[fence + shift:fence + shift + rows * n_out].view(rows, n_out)
    xs.copy_(x)
    for padtype in ("constant", "symmetric", "median"):
        ys.fill_(float("nan"))
        assert plan(xs, padtype, out=ys) is ys
        check(ys, signal.resample_poly(xw, 3, 2, axis=-1, padtype=padtype), dtype, f"fenced {padtype} shift {shift}")
        assert torch.isnan(ybuf[:fence + shift]).all() and torch.isnan(ybuf[fence + shift + rows * n_out:]).all()
        assert torch.isnan(xbuf[:fence + shift]).all() and torch.isnan(xbuf[fence + shift + rows * T:]).all()
        assert torch.equal(xs, x)


def test_round_trips(isd):
    x = rows_of(33, 37).reshape(3, 11, 37)
    xd = torch.tensor(x).cuda()
    same = isd.resample_poly(xd, 5, 5)                             # up == down: a copy that does not alias
    assert torch.equal(same, xd) and same.data_ptr() != xd.data_ptr()
    same = isd.resample_poly(x, 3, 3)
    assert isinstance(same, np.ndarray) and np.array_equal(same, x) and not np.shares_memory(same, x)
    for arr in (x, x.astype(np.float32)):                          # ndarray in -> computed in fp64 -> float64 ndarray out
        got = isd.resample_poly(arr, 3, 2, padtype="edge")
        ref = signal.resample_poly(arr.astype(np.float64), 3, 2, axis=-1, padtype="edge")
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == ref.shape
        assert rel_err(got, ref) <= 1e-12
    got = isd.resample_poly(x[0, 0], 2, 3)                         # [T]
    assert got.shape == (25,) and rel_err(got, signal.resample_poly(x[0, 0], 2, 3)) <= 1e-12
    got = isd.resample_poly(x, 2, 3, axis=1)                       # the channel axis: 11 -> 8
    assert got.shape == (3, 8, 37) and rel_err(got, signal.resample_poly(x, 2, 3, axis=1)) <= 1e-12
    got = isd.resample_poly(xd, 2, 3, axis=0, padtype="mean")
    assert tuple(got.shape) == (2, 11, 37)
    assert rel_err(got.cpu().numpy(), signal.resample_poly(x, 2, 3, axis=0, padtype="mean")) <= 1e-12
    for dtype in DTYPES:
        empty = isd.resample_poly(torch.empty(0, 11, 37, dtype=dtype, device="cuda"), 3, 2)
        assert tuple(empty.shape) == (0, 11, 56) and empty.dtype == dtype
    assert isd.resample_poly(np.empty((0, 37)), 3, 2).shape == (0, 56)


def test_resample_is_resample_poly_with_mne_defaults(isd):
    x = resample_ref.make_rows(6, 4096)
    for dtype in DTYPES:
        xd, xw = as_input(x, dtype)
        a = isd.resample(xd, up=250, down=1024)
        assert tuple(a.shape) == (6, 1000)
        assert torch.equal(a, isd.resample_poly(xd, 125, 512, padtype="reflect"))
        check(a, signal.resample_poly(xw, 125, 512, axis=-1, padtype="reflect"), dtype, "resample 250/1024")
        assert torch.equal(isd.resample(xd, 256.0, 1024.0, pad="edge"), isd.resample_poly(xd, 1, 4, padtype="edge"))
    got = isd.resample(x.reshape(2, 3, 4096), up=1, down=4, axis=-1)
    assert isinstance(got, np.ndarray) and got.shape == (2, 3, 1024)


def test_resampler_argument_errors(isd):
    plan = isd.Resampler(1, 2)
    x = torch.zeros(4, 37, device="cuda")
    assert plan.out_len(37) == 19 and tuple(plan(x).shape) == (4, 19)
    with pytest.raises(ValueError, match="out"):
        plan(x, out=torch.empty(4, 18, device="cuda"))
    with pytest.raises(ValueError, match="out"):
        plan(x, out=torch.empty(4, 19, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="out"):
        plan(x, out=torch.empty(4, 38, device="cuda")[:, ::2])
    with pytest.raises(ValueError, match="in-place"):
        isd.Resampler(1, 1)(x, out=x)
    with pytest.raises(TypeError):
        plan(x.cpu())
    with pytest.raises(TypeError):
        plan(x.half())
    with pytest.raises(ValueError, match="cval"):
        plan(x, "edge", cval=1.0)
    from isd_amd import _lib                                       # the library's own refusals
    import ctypes as C
    L = _lib.lib()
    y = torch.empty(4, 19, device="cuda")
    args = (C.c_void_p(torch.cuda.current_stream().cuda_stream),)
    assert L.isd_resample_poly_f32(plan._h, x.data_ptr(), y.data_ptr(), 4, 37, 5, 0.0, None, *args) == _lib.ISD_ERR_INVALID
    assert L.isd_resample_poly_f32(plan._h, x.data_ptr(), y.data_ptr(), 4, 1, 2, 0.0, None, *args) == _lib.ISD_ERR_INVALID
    assert L.isd_resample_poly_f32(plan._h, x.data_ptr(), x.data_ptr(), 4, 37, 0, 0.0, None, *args) == _lib.ISD_ERR_INVALID
    assert L.isd_resample_out_len(plan._h, 37) == 19
