"""NumPy float64 restatement of isd_amd.analytic.hilbert and isd_amd.connectivity.envelope_correlation, the data
generator and the cases that tests/test_envelope_cpu.py and tests/test_envelope_gpu.py share.

Per trial, z [C, T]: m = |z|, u = conj(z) / m (0 where m = 0), e = log(m^2) if log else m, ec = e - mean_t e,
se = |ec|_2 (1 where it is 0).  Pairwise: o[l, j, t] = |Im(z[l, t] u[j, t])| (log(o^2) if log), oc = o - mean_t o,
so = |oc|_2 (1 where 0), corr[l, j] = sum_t oc ec[j] / (se[j] so[l, j]), corr[l, l] = 0, result (A + A^T) / 2 with
A = |corr| if absolute else corr.  orthogonalize=False: corr[l, j] = sum_t ec[l] ec[j] / (se[l] se[j]).
"""
import numpy as np

# name -> (n, C, T); `long` (three staging chunks of the pair kernel plus 7) is added by the GPU tests
CASES = {
    "a": (3, 5, 65),
    "b": (2, 17, 250),
    "c": (2, 33, 795),           # odd length, three channel tiles with one channel in the last
    "c128": (1, 128, 64),
    "c1": (2, 1, 10),
    "t1": (2, 3, 1),
    "t2": (2, 3, 2),             # used real-valued
    "big": (300, 4, 128),
}


def make(n, C, T, seed):
    """x [n, C, T]: 0.6 w_c s(t) + noise_c(t), w ~ U(-1, 1) per channel, s and the noise standard normal; even channels
    are multiplied by 1 + 0.5 sin(2 pi 3 t / T + phi_trial), so some pairs have a real envelope correlation."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1.0, 1.0, C)
    s = rng.standard_normal((n, 1, T))
    x = 0.6 * w[None, :, None] * s + rng.standard_normal((n, C, T))
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    t = np.arange(T)
    x[:, ::2] *= (1.0 + 0.5 * np.sin(2.0 * np.pi * 3.0 * t[None] / T + phi[:, None]))[:, None, :]
    return x


def ref_hilbert(x, N=None):
    """scipy.signal.hilbert(x, N, axis=-1), restated."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[-1] if N is None else int(N)
    X = np.fft.fft(x, N, axis=-1)
    h = np.zeros(N)
    h[0] = 1.0
    if N % 2 == 0:
        h[N // 2] = 1.0
        h[1:N // 2] = 2.0
    else:
        h[1:(N + 1) // 2] = 2.0
    return np.fft.ifft(X * h, axis=-1)


def _centre(v):
    """v - mean_t v and its 2-norm with 1 where it is 0, along the last axis."""
    vc = v - v.mean(-1, keepdims=True)
    s = np.sqrt((vc * vc).sum(-1))
    return vc, np.where(s == 0, 1.0, s)


def ref_envcorr(z, orthogonalize="pairwise", log=False, absolute=True):
    """z complex [n, C, T] (or [C, T]) -> [n, C, C] float64."""
    z = np.asarray(z, dtype=np.complex128)
    if z.ndim == 2:
        return ref_envcorr(z[None], orthogonalize, log, absolute)[0]
    n, C, T = z.shape
    out = np.zeros((n, C, C))
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(n):
            zi = z[i]
            m = np.abs(zi)
            u = np.where(m == 0, 0.0, np.conj(zi) / np.where(m == 0, 1.0, m))
            e = np.log(m * m) if log else m
            ec, se = _centre(e)
            if orthogonalize is False:
                out[i] = (ec @ ec.T) / (se[:, None] * se[None, :])
                continue
            corr = np.zeros((C, C))
            for j in range(C):
                o = np.abs((zi * u[j][None, :]).imag)                   # o[l, t] = o[l | j]
                if log:
                    o = np.log(o * o)
                oc, so = _centre(o)
                corr[:, j] = (oc * ec[j][None, :]).sum(-1) / (se[j] * so)
            corr[np.arange(C), np.arange(C)] = 0.0
            A = np.abs(corr) if absolute else corr
            out[i] = (A + A.T) / 2
    return out
