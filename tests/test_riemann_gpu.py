"""GPU parity of isd_amd.riemann (csrc/riemann.hip, isd_amd/riemann.py).

The eigen kernel is checked against a CONSTRUCTED spectrum, A = Q diag(λ) Qᵀ with the reference Q f(λ) Qᵀ, which
involves no eigensolver.  Bounds on max|Δ| / max|ref| per matrix: 1e-10 for κ <= 1e4 and 1e-8 for κ = 1e6, about
50 ε κ: a NumPy prototype of the same one-sided Jacobi gave <= 2.7e-14 / 1.2e-12 for log and <= 1.3e-13 / 1.2e-11 for
1/sqrt, and NumPy's eigh the same, so a wrong rotation or a lost column misses them by ten orders.  The congruence
is checked against np.einsum (1e-13), the functions and estimators against the NumPy / SciPy restatement of
tests/riemann_ref.py (tangent vectors and distances 1e-10, means 1e-9 and the same iteration count).
Measured on an MI355X (worst over the cases below): see DESIGN.md §3.14."""
import ctypes

import numpy as np
import pytest
import torch

import riemann_ref as ref

pytestmark = pytest.mark.gpu

KAPPAS = [1e2, 1e4, 1e6]
EIG_SHAPES = [(1, 1), (1, 2), (3, 3), (130, 9), (2, 16), (2, 17), (2, 33), (3, 64), (2, 65), (2, 128)]
FNS = {"log": np.log, "sqrt": np.sqrt, "invsqrt": lambda v: 1.0 / np.sqrt(v), "inv": lambda v: 1.0 / v}


def bound(kappa):
    return 1e-10 if kappa <= 1e4 else 1e-8


@pytest.fixture(scope="module")
def rm():
    from isd_amd import riemann
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return riemann


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.array(a), dtype=dtype).cuda()               # a copy: the shared references stay read-only


def host(t):
    return t.detach().cpu().numpy()


def worst_rel(got, want):
    """max over the batch of max|Δ| / max|ref| per matrix (or per row)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    n = len(want)
    num = np.abs(got - want).reshape(n, -1).max(1)
    den = np.maximum(np.abs(want).reshape(n, -1).max(1), 1e-300)
    return float((num / den).max())


def constructed(n, C, kappa, seed=0):
    """-> (A [n, C, C], Q [n, C, C], lam [n, C]): A_i = Q_i diag(lam_i) Q_iᵀ, symmetrised; lam log-spaced over kappa
    and scaled per matrix."""
    rng = np.random.default_rng(seed + 1000 * C + n)
    Q = np.stack([np.linalg.qr(rng.standard_normal((C, C)))[0] for _ in range(n)])
    base = np.logspace(0, -np.log10(kappa), C) if C > 1 else np.ones(1)
    lam = base[None, :] * (0.7 + 0.45 * (np.arange(n) % 7))[:, None]
    return assemble(Q, lam), Q, lam


def assemble(Q, lam):
    A = np.einsum("nab,nb,ncb->nac", Q, lam, Q)
    return (A + A.transpose(0, 2, 1)) / 2


def check_functions(rm, A, Q, lam, kappa, label):
    """Every fn x out of spd_function on A against Q f(lam) Qᵀ, eigenvalues, info, symmetry.  Returns the worst."""
    Ad = dev(A)
    worst = {}
    for name, f in FNS.items():
        want = assemble(Q, f(lam))
        full, info = rm.spd_function(Ad, name, out="full", return_info=True)
        assert bool((info > 0).all()), f"{label} {name}: info {host(info)}"
        assert torch.equal(full, full.mT), f"{label} {name}: FULL output is not bit-symmetric"
        tang = rm.spd_function(Ad, name, out="tangent")
        assert tang.shape == (len(A), A.shape[1] * (A.shape[1] + 1) // 2)
        e_full, e_tang = worst_rel(host(full), want), worst_rel(host(tang), ref.upper(want))
        print(f"{label} {name}: full {e_full:.3g} tangent {e_tang:.3g} sweeps <= {int(info.max())}")
        worst[name] = max(e_full, e_tang)
    eig = host(rm.spd_eigvalsh(Ad))
    e_eig = float((np.abs(eig - np.sort(lam, axis=1)).max(1) / lam.max(1)).max())
    print(f"{label} eigvals: {e_eig:.3g}")
    assert e_eig <= 1e-13
    for name, e in worst.items():
        assert e <= bound(kappa), f"{label} {name}: {e:.3g} > {bound(kappa):g}"
    return worst


# ---------------------------------------------------------------------------------- 1. constructed spectra
@pytest.mark.parametrize("kappa", KAPPAS)
@pytest.mark.parametrize("n,C", EIG_SHAPES)
def test_eigfun_constructed_spectrum(rm, n, C, kappa):
    A, Q, lam = constructed(n, C, kappa)
    check_functions(rm, A, Q, lam, kappa, f"n={n} C={C} kappa={kappa:g}")


# ---------------------------------------------------------------------------------- 2. degenerate spectra
def test_eigfun_degenerate_spectra(rm):
    rng = np.random.default_rng(3)
    # the identity and a diagonal matrix: no rotation at all, one sweep
    for C_, lam in ((9, np.ones(9)), (17, np.linspace(0.5, 4.0, 17))):
        Q = np.eye(C_)[None]
        check_functions(rm, assemble(Q, lam[None]), Q, lam[None], 1e2, f"diag C={C_}")
        _, info = rm.spd_function(dev(np.diag(lam)[None]), "log", return_info=True)
        assert int(info[0]) == 1
    # eigenvalues repeated in clusters of 3 (any basis of a cluster's eigenspace is right: f(A) is still unique)
    for C_ in (12, 33):
        Q = np.linalg.qr(rng.standard_normal((C_, C_)))[0][None]
        lam = np.repeat(np.logspace(0, -2, C_ // 3), 3)[None]
        check_functions(rm, assemble(Q, lam), Q, lam, 1e2, f"clusters C={C_}")
    # columns that are already mutually orthogonal (G = V Λ at the start).  For a symmetric positive-definite A,
    # AᵀA = A² diagonal forces A to be diagonal with blocks c I, so this is a diagonal matrix with repeated entries
    # in scattered positions: γ = 0 at every pair and α = β (ζ = 0 / 0 if the skip test were missing) inside a block
    lam = np.repeat([2.0, 0.5, 0.125, 3.0], [5, 4, 3, 4])
    perm = rng.permutation(16)
    Q = np.eye(16)[perm][None]
    check_functions(rm, assemble(Q, lam[None]), Q, lam[None], 1e2, "orthogonal columns C=16")
    _, info = rm.spd_function(dev(assemble(Q, lam[None])), "sqrt", return_info=True)
    assert int(info[0]) == 1


# ------------------------------------------------------------------------------------------- 3. isolation
PAD = 96


def fenced(shape, dtype=torch.float64, fill=None):
    """A contiguous view of `shape` inside a larger NaN-filled device buffer (int buffers: -77 sentinels)."""
    size = int(np.prod(shape))
    sentinel = float("nan") if dtype.is_floating_point else -77
    buf = torch.full((size + 2 * PAD,), sentinel, dtype=dtype, device="cuda")
    view = buf[PAD:PAD + size].view(shape)
    if fill is not None:
        view.copy_(torch.as_tensor(fill))
    return buf, view


def fences_intact(buf, size):
    edge = torch.cat([buf[:PAD], buf[PAD + size:]])
    return bool(torch.isnan(edge).all()) if buf.dtype.is_floating_point else bool((edge == -77).all())


def raw_eigfun(A, fn, kind):
    """isd_spd_eigfun on fenced buffers -> (out, eigvals, info) as host arrays; checks every fence."""
    from isd_amd import _lib
    n, C_, _ = A.shape
    width = {0: C_ * C_, 1: C_ * (C_ + 1) // 2, 2: 1}[kind]
    abuf, a = fenced(A.shape, fill=A)
    obuf, out = fenced((n, width))
    ebuf, eig = fenced((n, C_))
    ibuf, info = fenced((n,), dtype=torch.int32)
    _lib.check(_lib.lib().isd_spd_eigfun(a.data_ptr(), out.data_ptr() if kind != 2 else None, eig.data_ptr(),
                                         info.data_ptr(), n, C_, fn, kind,
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for b, size in ((abuf, A.size), (obuf, n * width), (ebuf, n * C_), (ibuf, n)):
        assert fences_intact(b, size), "wrote outside a buffer"
    assert torch.equal(a.view(torch.int64), dev(A).view(torch.int64)), "the input was modified"
    if kind == 2:
        assert bool(torch.isnan(out).all()), "NOOUT wrote to out"
    return host(out), host(eig), host(info)


@pytest.mark.parametrize("n,C", [(5, 3), (6, 9), (4, 17), (3, 33), (3, 64), (3, 65)])
def test_eigfun_isolation_and_repeatability(rm, n, C):
    A, _, lam = constructed(n, C, 1e3, seed=5)
    for fn, kind in ((rm.SPD_LOG, rm.SPD_FULL), (rm.SPD_INVSQRT, rm.SPD_TANGENT), (rm.SPD_LOG, rm.SPD_NOOUT)):
        out, eig, info = raw_eigfun(A, fn, kind)
        assert (info > 0).all()
        assert np.isfinite(eig).all() and (kind == rm.SPD_NOOUT or np.isfinite(out).all()), "read a NaN sentinel"
        out2, eig2, info2 = raw_eigfun(A, fn, kind)                  # a second call: the same bits
        assert np.array_equal(out, out2, equal_nan=True) and np.array_equal(eig, eig2) and np.array_equal(info, info2)
        perm = np.random.default_rng(n + C).permutation(n)           # a permuted batch: the same bits per matrix
        outp, eigp, infop = raw_eigfun(A[perm], fn, kind)
        assert np.array_equal(outp, out[perm], equal_nan=True) and np.array_equal(eigp, eig[perm])
        assert np.array_equal(infop, info[perm])
        out1, eig1, info1 = raw_eigfun(A[n - 1:], fn, kind)          # a matrix alone
        assert np.array_equal(out1[0], out[n - 1], equal_nan=True) and np.array_equal(eig1[0], eig[n - 1])
        assert info1[0] == info[n - 1]


@pytest.mark.parametrize("C", [4, 9, 33, 64])
def test_eigfun_bad_matrices_end_and_do_not_touch_their_neighbours(rm, C):
    """Input validation with bounded loops: a NaN, an indefinite and a singular matrix each end with info < 0 and a
    NaN result; nothing outside the buffers is read or written; the good matrices come out as in a clean batch."""
    good, Q, lam = constructed(4, C, 1e3, seed=9)
    nan_m = good[0].copy()
    nan_m[1, 2] = nan_m[2, 1] = np.nan
    indef_diag = np.diag(np.where(np.arange(C) % 2 == 0, 1.0, -1.0))
    lam_neg = lam[1].copy()
    lam_neg[C // 2] *= -1.0
    indef_full = assemble(Q[1:2], lam_neg[None])[0]
    singular = good[2].copy()
    singular[1, :] = 0.0
    singular[:, 1] = 0.0
    batch = np.stack([good[0], nan_m, good[1], indef_diag, good[2], indef_full, singular, good[3]])
    bad_at, good_at = [1, 3, 5, 6], [0, 2, 4, 7]
    clean_full, clean_eig, clean_info = raw_eigfun(good, rm.SPD_LOG, rm.SPD_FULL)
    clean_tang, _, _ = raw_eigfun(good, rm.SPD_LOG, rm.SPD_TANGENT)
    full, eig, info = raw_eigfun(batch, rm.SPD_LOG, rm.SPD_FULL)
    tang, _, info_t = raw_eigfun(batch, rm.SPD_LOG, rm.SPD_TANGENT)
    print(f"C={C}: info {info}")
    assert np.array_equal(info, info_t)
    assert all(info[i] in (-1, -2) for i in bad_at), info
    assert np.isnan(full[bad_at]).all() and np.isnan(tang[bad_at]).all()
    assert np.array_equal(full[good_at], clean_full) and np.array_equal(tang[good_at], clean_tang)
    assert np.array_equal(eig[good_at], clean_eig) and np.array_equal(info[good_at], clean_info)
    with pytest.raises(ValueError, match="matrix 1 "):
        rm.spd_function(dev(batch), "log")
    with pytest.raises(ValueError, match="matrix 0 "):
        rm.spd_function(dev(batch[6:]), "log", out="tangent")      # the singular matrix
    with pytest.raises(ValueError, match="matrix 1 "):
        rm.spd_eigvalsh(dev(batch[2:4]))                             # indefinite: not a question of the function


@pytest.mark.parametrize("n,C", [(4096, 16), (1536, 64), (520, 128)])
def test_eigfun_full_card_batch_repeats_its_matrices(rm, n, C):
    """More workgroups than the card holds at once, cycling through five matrices: every copy comes out as the matrix
    does alone.  Waves of one workgroup run far apart under this load, which is when an unordered access to the
    shared matrix shows."""
    A, _, _ = constructed(5, C, 1e2, seed=21)
    alone_full, alone_info = rm.spd_function(dev(A), "log", return_info=True)
    alone_eig = rm.spd_eigvalsh(dev(A))
    pick = torch.arange(n, device="cuda") % 5
    big = dev(A)[pick].contiguous()
    tang, info = rm.spd_function(big, "log", out="tangent", return_info=True)
    assert bool((info > 0).all()), f"{int((info <= 0).sum())} of {n} matrices failed"
    assert torch.equal(info, alone_info[pick])
    iu = torch.triu_indices(C, C, device="cuda")
    coef = torch.full((iu.shape[1],), 2.0 ** 0.5, dtype=torch.float64, device="cuda")
    coef[iu[0] == iu[1]] = 1.0
    assert torch.equal(tang, (alone_full[:, iu[0], iu[1]] * coef)[pick])
    assert torch.equal(rm.spd_eigvalsh(big), alone_eig[pick])
    W = dev(np.random.default_rng(C).standard_normal((3, C, C)))
    widx = (torch.arange(n) % 3).numpy()
    got = rm.congruence(big, W, widx)
    small = torch.stack([rm.congruence(dev(A), W[k:k + 1]) for k in range(3)])        # [3, 5, C, C]
    assert torch.equal(got, small[torch.as_tensor(widx).cuda(), pick])


def test_eigfun_rejects_bad_calls(rm):
    from isd_amd import _lib
    L = _lib.lib()
    a = torch.eye(4, dtype=torch.float64, device="cuda")[None].contiguous()
    out = torch.empty_like(a)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.isd_spd_eigfun(a.data_ptr(), out.data_ptr(), None, None, 0, 4, 0, 0, st) == 0          # n = 0
    assert L.isd_spd_eigfun(a.data_ptr(), None, None, None, 1, 4, 0, 2, st) == 0                    # NOOUT, no out
    assert L.isd_spd_eigfun(None, out.data_ptr(), None, None, 1, 4, 0, 0, st) == _lib.ISD_ERR_INVALID
    assert L.isd_spd_eigfun(a.data_ptr(), None, None, None, 1, 4, 0, 0, st) == _lib.ISD_ERR_INVALID
    assert L.isd_spd_eigfun(a.data_ptr(), a.data_ptr(), None, None, 1, 4, 0, 0, st) == _lib.ISD_ERR_INVALID
    assert L.isd_spd_eigfun(a.data_ptr(), out.data_ptr(), None, None, 1, 0, 0, 0, st) == _lib.ISD_ERR_INVALID
    assert L.isd_spd_eigfun(a.data_ptr(), out.data_ptr(), None, None, 1, 4, 5, 0, st) == _lib.ISD_ERR_INVALID
    assert L.isd_spd_eigfun(a.data_ptr(), out.data_ptr(), None, None, 1, 4, 0, 3, st) == _lib.ISD_ERR_INVALID
    assert L.isd_spd_eigfun(a.data_ptr(), out.data_ptr(), None, None, 1, 129, 0, 0, st) == _lib.ISD_ERR_UNSUPPORTED
    assert L.isd_spd_congruence(a.data_ptr(), 1, a.data_ptr(), None, out.data_ptr(), 1, 129, 1, st) \
        == _lib.ISD_ERR_UNSUPPORTED
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 4. congruence
@pytest.mark.parametrize("n,C,K", [(1, 1, 1), (3, 9, 2), (130, 9, 3), (2, 17, 1), (2, 64, 5), (2, 128, 2),
                                   (2, 33, 2), (3, 80, 2), (2, 100, 1), (2, 113, 2)])       # every tile count 1 .. 8
def test_congruence_against_einsum(rm, n, C, K):
    from isd_amd import _lib
    rng = np.random.default_rng(100 * n + C + K)
    cov64 = ref.covariances(ref.synthetic_trials(n, C, 4 * C + 1, seed=n + C))
    W = rng.standard_normal((K, C, C)) + np.eye(C)                   # not symmetric: a transposed product would show
    widx = rng.integers(0, K, size=n)
    widx[-1] = K - 1
    for dtype in (torch.float64, torch.float32):
        cbuf, cov = fenced((n, C, C), dtype=dtype, fill=cov64)
        wbuf, Wd = fenced((K, C, C), fill=W)
        cov_h = host(cov).astype(np.float64)                         # what the kernel reads, exactly
        for idx in (widx, None):
            sel = W[widx] if idx is not None else np.broadcast_to(W[0], (n, C, C))
            want = np.einsum("nab,nbc,ndc->nad", sel, cov_h, sel)
            got = rm.congruence(cov, Wd, idx)
            assert got.shape == (n, C, C) and got.dtype == torch.float64
            assert bool(torch.isfinite(got).all()), "read a NaN sentinel"
            assert torch.equal(got, got.mT), "not exactly symmetric"
            err = worst_rel(host(got), want)
            print(f"congruence n={n} C={C} K={K} {dtype} widx={'given' if idx is not None else 'NULL'}: {err:.3g}")
            assert err <= 1e-13
        # the raw call into a fenced output: nothing outside it is written
        obuf, out = fenced((n, C, C))
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib().isd_spd_congruence(cov.data_ptr(), int(dtype == torch.float64), Wd.data_ptr(), None,
                                                 out.data_ptr(), n, C, K, st))
        torch.cuda.synchronize()
        assert fences_intact(obuf, n * C * C) and torch.equal(out, got)
        if dtype == torch.float64:                                   # an aliased output is rejected
            rc = _lib.lib().isd_spd_congruence(cov.data_ptr(), 1, Wd.data_ptr(), None, cov.data_ptr(), n, C, K, st)
            assert rc == _lib.ISD_ERR_INVALID
    with pytest.raises(ValueError):
        rm.congruence(cov, Wd, np.full(n, K))                        # widx outside [0, K)


# ------------------------------------------------------------ 5. tangent space, distance, mean vs the restatement
PIPE_SHAPES = [(6, 8, 250), (5, 12, 129), (8, 16, 257), (4, 64, 795), (2, 128, 1030)]
_pipe_cache = {}


def pipe_case(n, C, T):
    """Covariances of synthetic trials and everything the restatement says about them, computed once."""
    key = (n, C, T)
    if key not in _pipe_cache:
        covs = ref.covariances(ref.synthetic_trials(n, C, T, seed=C + T))
        mean, iters = ref.mean_riemann(covs)
        other = ref.covariances(ref.synthetic_trials(2, C, T, seed=C + T + 1))
        for a in (covs, mean, other):
            a.setflags(write=False)
        _pipe_cache[key] = dict(covs=covs, mean=mean, iters=iters, other=other,
                                tangent=ref.tangent_space(covs, mean),
                                dist=ref.distances(covs, np.concatenate([mean[None], other])))
    return _pipe_cache[key]


@pytest.mark.parametrize("n,C,T", PIPE_SHAPES)
def test_tangent_space_and_distance(rm, n, C, T):
    case = pipe_case(n, C, T)
    covs = dev(case["covs"])
    t = rm.tangent_space(covs, case["mean"])
    assert t.shape == (n, C * (C + 1) // 2) and t.dtype == torch.float64 and t.is_cuda
    e_t = float(np.abs(host(t) - case["tangent"]).max() / np.abs(case["tangent"]).max())
    refs = np.concatenate([case["mean"][None], case["other"]])
    d = rm.distance_riemann(covs, refs)
    assert d.shape == (n, 3)
    e_d = float(np.abs(host(d) - case["dist"]).max() / np.abs(case["dist"]).max())
    d0 = rm.distance_riemann(covs, case["mean"])
    assert d0.shape == (n,) and torch.equal(d0, d[:, 0])
    # the norm of a tangent vector is the distance to the reference
    e_n = float((torch.linalg.norm(t, dim=1) - d0).abs().max() / d0.max())
    print(f"n={n} C={C} T={T}: tangent {e_t:.3g} distance {e_d:.3g} norm-vs-distance {e_n:.3g}")
    assert e_t <= 1e-10 and e_d <= 1e-10 and e_n <= 1e-10
    assert torch.equal(rm.tangent_space(case["covs"], case["mean"]), t)          # ndarray in: the same bits


@pytest.mark.parametrize("n,C,T", PIPE_SHAPES)
def test_mean_riemann(rm, n, C, T):
    case = pipe_case(n, C, T)
    M, iters = rm.mean_riemann(dev(case["covs"]), return_n_iter=True)
    assert M.shape == (C, C) and M.dtype == np.float64 and np.array_equal(M, M.T)
    err = float(np.abs(M - case["mean"]).max() / np.abs(case["mean"]).max())
    W = ref.invsqrtm(M)                                              # stationarity, independent of the restatement's mean
    grad = sum(ref.logm(W @ c @ W) for c in case["covs"])
    station = float(np.linalg.norm(grad) / n)
    print(f"n={n} C={C} T={T}: mean {err:.3g} iterations {iters} (restatement {case['iters']}) stationarity "
          f"{station:.3g}")
    assert iters == case["iters"]
    assert err <= 1e-9
    assert station <= 1e-7


@pytest.mark.parametrize("n,C,T,labels", [(6, 8, 250, [1, 0, 1, 0, 2, 2]), (8, 16, 257, [5, 5, 3, 3, 3, 5, 9, 5])])
def test_mean_riemann_groups_equal_separate_calls(rm, n, C, T, labels):
    case = pipe_case(n, C, T)
    covs, labels = dev(case["covs"]), np.array(labels)
    w = np.linspace(0.5, 2.0, n)
    for sw in (None, w):
        means, iters = rm.mean_riemann(covs, groups=labels, sample_weight=sw, return_n_iter=True)
        classes = np.unique(labels)
        assert means.shape == (len(classes), C, C) and iters.shape == (len(classes),)
        for k, c in enumerate(classes):
            sel = np.flatnonzero(labels == c)
            alone, it = rm.mean_riemann(covs[torch.as_tensor(sel).cuda()], sample_weight=None if sw is None else sw[sel],
                                        return_n_iter=True)
            assert np.array_equal(alone, means[k]), f"class {c}: the grouped mean differs from the mean alone"
            assert it == iters[k]
            want, _ = ref.mean_riemann(case["covs"][sel], sample_weight=None if sw is None else sw[sel])
            assert np.abs(means[k] - want).max() <= 1e-9 * np.abs(want).max()


# ------------------------------------------------------------------------------------------- 6. estimators
@pytest.fixture(scope="module")
def three_class():
    X, y = ref.three_class_trials()
    covs = ref.covariances(X)
    classes, means, _ = ref.class_means(covs, y)
    d = ref.distances(covs, means)
    for a in (X, covs, means, d):
        a.setflags(write=False)
    return dict(X=X, y=y, covs=covs, classes=classes, means=means, dist=d, tangent=ref.tangent_space(
        covs, ref.mean_riemann(covs)[0]))


def test_covariances_tangent_space_kinds(rm, three_class):
    X, want = three_class["X"], three_class["tangent"]
    got = rm.TangentSpace().fit_transform(rm.Covariances().fit_transform(X))
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    # fp32 trials: the covariances carry the fp32 kernel's error, bounded by 1e-5 max|C| in test_csp_gpu.py.  Whitened
    # by M^-1/2 that is at most 1e-5 ‖C‖ / λ_min(M) in norm, and log has Lipschitz constant 1 / λ_min of the whitened
    # matrix; the reference point moves by the same order.  Factor 4: trial + reference + the √2 of the off-diagonal
    # entries, rounded up.  All of it from the reference's own numbers.
    M = ref.mean_riemann(three_class["covs"])[0]
    Wm = ref.invsqrtm(M)
    lam_w = min(np.linalg.eigvalsh(Wm @ c @ Wm)[0] for c in three_class["covs"])
    amp = max(np.linalg.norm(c, 2) for c in three_class["covs"]) / np.linalg.eigvalsh(M)[0]
    # round trip through inverse_transform (back to the covariances that went in): a perturbation E of the tangent
    # vector S, here its rounding to the tensor's dtype, moves exp(S) by at most ‖E‖ e^‖E‖ ‖exp S‖ and the covariance
    # by κ(M) times that relative to its norm; norm to entry costs a factor C = 8; + 1 for rounding the result
    kappa_m, s_max = np.linalg.cond(M), np.linalg.norm(want, axis=1).max()
    cases = ((torch.float64, 1e-10, 1e-10 * kappa_m * 8),
             (torch.float32, 4e-5 * amp / lam_w, 2.0 ** -24 * (s_max * kappa_m * 8 + 1)))
    for dtype, tol, tol_back in cases:
        xd = dev(X, dtype)
        covs = rm.Covariances().transform(xd)
        assert covs.is_cuda and covs.dtype == dtype and covs.shape == (90, 8, 8)
        ts = rm.TangentSpace().fit(covs)
        assert isinstance(ts.reference_, np.ndarray) and ts.reference_.dtype == np.float64
        t = ts.transform(covs)
        assert t.is_cuda and t.device == xd.device and t.dtype == dtype and t.shape == want.shape
        err = float(np.abs(host(t).astype(np.float64) - want).max())
        back = ts.inverse_transform(t)
        assert back.is_cuda and back.dtype == dtype
        err_back = float((back - covs).abs().max() / covs.abs().max())
        print(f"Covariances -> TangentSpace {dtype}: {err:.3g} (bound {tol:.3g}); round trip {err_back:.3g} "
              f"(bound {tol_back:.3g})")
        assert err <= tol * (np.abs(want).max() if dtype == torch.float64 else 1.0)
        assert err_back <= tol_back


def test_mdm_against_restatement(rm, three_class):
    covs, y, d_ref = three_class["covs"], three_class["y"], three_class["dist"]
    mdm = rm.MDM().fit(covs, y)
    assert np.array_equal(mdm.classes_, three_class["classes"]) and mdm.covmeans_.shape == (3, 8, 8)
    assert np.abs(mdm.covmeans_ - three_class["means"]).max() <= 1e-9 * np.abs(three_class["means"]).max()
    d = mdm.transform(covs)
    assert isinstance(d, np.ndarray) and d.shape == (90, 3)
    # triangle inequality: the distance kernel's own 1e-10, plus how far each fitted mean lies from the restatement's
    shift = np.array([ref.distance(mdm.covmeans_[k], three_class["means"][k]) for k in range(3)])
    print(f"MDM distances: {np.abs(d - d_ref).max():.3g}; means moved by {shift.max():.3g}")
    assert np.all(np.abs(d - d_ref) <= 1e-10 * d_ref.max() + shift[None, :])
    srt = np.sort(d_ref, axis=1)
    decided = (srt[:, 1] - srt[:, 0]) > 1e-6
    excluded = int((~decided).sum())
    assert excluded == 0
    pred = mdm.predict(covs)
    assert np.array_equal(pred[decided], three_class["classes"][np.argmin(d_ref, axis=1)][decided])
    proba = mdm.predict_proba(covs)
    assert proba.shape == (90, 3) and np.abs(proba.sum(1) - 1.0).max() <= 1e-12
    assert np.array_equal(np.argmax(proba, axis=1), np.argmin(d, axis=1))
    assert mdm.score(covs, y) == float(np.mean(pred == y))
    # labels that are not 0..K-1, a CUDA tensor in -> a CUDA tensor out, weights
    names = np.array(["rest", "left", "right"])[y]
    covs_d = dev(covs)
    mdm2 = rm.MDM().fit(covs_d, names, sample_weight=np.ones(90))
    assert list(mdm2.classes_) == sorted(set(names))
    assert np.array_equal(mdm2.predict(covs_d) == "left", pred == 1)
    dd = mdm2.transform(covs_d)
    assert dd.is_cuda and dd.dtype == torch.float64 and dd.shape == (90, 3)
    # ties go to the lowest class
    mdm2.covmeans_ = np.stack([mdm.covmeans_[0]] * 3)
    assert set(mdm2.predict(covs_d)) == {mdm2.classes_[0]}


def test_readme_pipelines_under_sklearn(rm, three_class):
    pipe = pytest.importorskip("sklearn.pipeline")
    base = pytest.importorskip("sklearn.base")
    lm = pytest.importorskip("sklearn.linear_model")
    X, y = three_class["X"], three_class["y"]
    clf = base.clone(pipe.make_pipeline(rm.Covariances(), rm.TangentSpace(), lm.LogisticRegression())).fit(X, y)
    mdm = base.clone(pipe.make_pipeline(rm.Covariances(), rm.MDM())).fit(X, y)
    assert clf.score(X, y) > 0.9 and mdm.score(X, y) > 0.9
    assert clf.predict(X[:7]).shape == (7,) and mdm.predict_proba(X[:7]).shape == (7, 3)
