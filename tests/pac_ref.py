"""NumPy float64 restatement of isd_amd.pac (the definitions of its module docstring), the case table and the data
generator that tests/test_pac_cpu.py and tests/test_pac_gpu.py share.

For one row: phi_p[t] in [-pi, pi], a_q[t] >= 0, a_q^s[t] = a_q[(t + s) mod T], B bins,
b[t] = min(B - 1, max(0, floor((double(phi[t]) + pi) * c))) with c = B / (2 pi), n_j the samples of bin j.
  mvl = |sum_t a^s[t] exp(i phi[t])| / T
  mi  = 1 + sum_{j: P_j > 0} P_j log P_j / log B,  P_j = m_j / sum_k m_k,  m_j = (sum_{b[t] = j} a^s[t]) / n_j or 0
  hr  = (max_j m_j - min_j m_j) / max_j m_j
Shift 0 is the estimate, the others are surrogates: mean, population std, n_ge = #{i >= 1: v(s_i) >= v(0)}.
"""
import numpy as np

METHODS = ("mvl", "mi", "hr")        # the order of the kernel's method axis


def ref_bins(phi, n_bins):
    """The phase bin of every sample, as integers; the expression of the definition, in float64."""
    c = n_bins / (2.0 * np.pi)
    b = np.floor((np.asarray(phi).astype(np.float64) + np.pi) * c)
    return np.minimum(n_bins - 1, np.maximum(0, b)).astype(np.int64)


def ref_pac(pha, amp, shifts, n_bins):
    """pha [P, T], amp [A, T], shifts [1 + S] -> (mvl, mi, hr), each [A, P, 1 + S] float64."""
    pha = np.asarray(pha, dtype=np.float64)
    amp = np.asarray(amp, dtype=np.float64)
    shifts = np.asarray(shifts, dtype=np.int64)
    (P, T), A, B = pha.shape, amp.shape[0], int(n_bins)
    assert amp.shape[1] == T and (shifts >= 0).all() and (shifts < T).all()
    a_s = amp[:, (np.arange(T)[None, :] + shifts[:, None]) % T]          # [A, 1 + S, T]: a[(t + s) mod T]
    mvl, mi, hr = (np.zeros((A, P, shifts.size)) for _ in range(3))
    with np.errstate(divide="ignore", invalid="ignore"):
        for p in range(P):
            b = ref_bins(pha[p], B)
            onehot = (b[:, None] == np.arange(B)[None, :]).astype(np.float64)    # [T, B]
            n_j = onehot.sum(0)
            mvl[:, p] = np.abs(a_s @ np.exp(1j * pha[p])) / T
            m = np.where(n_j > 0, (a_s @ onehot) / np.where(n_j > 0, n_j, 1.0), 0.0)     # [A, 1 + S, B]
            Pj = m / m.sum(-1, keepdims=True)
            plogp = np.where(Pj > 0, Pj * np.log(np.where(Pj > 0, Pj, 1.0)), 0.0)
            mi[:, p] = 1.0 + plogp.sum(-1) / np.log(B) + 0.0 * Pj.sum(-1)               # NaN where sum_k m_k = 0
            hr[:, p] = (m.max(-1) - m.min(-1)) / m.max(-1)
    return mvl, mi, hr


def ref_stats(v):
    """v [..., 1 + S] -> (surr_mean, surr_std, n_ge) over the surrogates v[..., 1:]; NaN, NaN, 0 without any."""
    s = v[..., 1:]
    if s.shape[-1] == 0:
        nan = np.full(v.shape[:-1], np.nan)
        return nan, nan.copy(), np.zeros(v.shape[:-1])
    return s.mean(-1), s.std(-1), (s >= v[..., :1]).sum(-1).astype(np.float64)


def ref_block(pha, amp, shifts, n_bins):
    """pha [rows, P, T], amp [rows, A, T] -> (block [rows, A, P, 3, 4], surr [rows, A, P, 3, S]): the layout of
    isd_amd.pac.pac_launch."""
    rows, S = pha.shape[0], len(shifts) - 1
    A, P = amp.shape[1], pha.shape[1]
    block, surr = np.zeros((rows, A, P, 3, 4)), np.zeros((rows, A, P, 3, S))
    for r in range(rows):
        for m, v in enumerate(ref_pac(pha[r], amp[r], shifts, n_bins)):
            mean, std, n_ge = ref_stats(v)
            block[r, :, :, m] = np.stack([v[..., 0], mean, std, n_ge], -1)
            surr[r, :, :, m] = v[..., 1:]
    return block, surr


# case -> rows, P, A, T, S, n_bins, seed.  The seeds of cases 1, 3 and 4 were picked on the CPU so that no surrogate
# value of the float64 restatement of the float32-rounded inputs comes within GAP of its estimate (test_pac_gpu.py
# asserts it): the count n_ge is then decided by the tolerance a hundred times over.  The one exception is 'hr' of case
# 1: 37 samples leave some of 18 bins empty in every row, so min_j m_j = 0 and hr is exactly 1 for the estimate and for
# every surrogate, in any precision; there the test asserts exactly that instead of a gap.
CASES = {
    1: dict(rows=3, P=2, A=3, T=37, S=5, B=18, seed=0),
    2: dict(rows=1, P=1, A=1, T=1, S=0, B=18, seed=2),
    3: dict(rows=2, P=1, A=2, T=129, S=64, B=18, seed=11165),          # 65 shifts: one lane past a wave
    4: dict(rows=1, P=1, A=1, T=795, S=200, B=18, seed=1043),
    5: dict(rows=2, P=2, A=1, T=64, S=3, B=2, seed=5),
    6: dict(rows=2, P=2, A=1, T=64, S=3, B=64, seed=6),
    7: dict(rows=1, P=2, A=2, T=100, S=4, B=18, seed=7),               # phases confined to [0, pi / 2]: empty bins
    8: dict(rows=1, P=1, A=1, T=4096, S=3, B=18, seed=8),              # shifts {0, 1, 2048, 4095}
    9: dict(rows=300, P=1, A=1, T=16, S=2, B=18, seed=9),              # grid indexing
    10: dict(rows=1, P=1, A=2, T=20, S=1, B=18, seed=10),              # phi holds -pi, +pi, float32(pi) and 0.0
}
GAP_CASES = (1, 3, 4)
GAP = {"mvl": 6e-4, "mi": 2e-4, "hr": 1e-3}       # what the seeds of GAP_CASES were picked for


def make_case(case, dtype=np.float64, seed=None):
    """-> (pha [rows, P, T], amp [rows, A, T], shifts int32 [1 + S], n_bins): phi = U(-pi, pi), a = |1 + N(0, 1)|,
    shifts uniform on [1, T - 1]; rounded to ``dtype`` and widened to float64 again."""
    k = CASES[case]
    rng = np.random.default_rng(k["seed"] if seed is None else seed)
    rows, P, A, T, S = k["rows"], k["P"], k["A"], k["T"], k["S"]
    pha = rng.uniform(-np.pi, np.pi, (rows, P, T))
    amp = np.abs(1.0 + rng.standard_normal((rows, A, T)))
    shifts = np.zeros(1 + S, dtype=np.int32)
    if S:
        shifts[1:] = rng.integers(1, T, size=S)
    if case == 7:
        pha = (pha + np.pi) / 4.0                                       # [0, pi / 2]
    if case == 8:
        shifts[:] = [0, 1, 2048, 4095]
    if case == 10:
        pha[0, 0, :4] = [-np.pi, np.pi, np.float64(np.float32(np.pi)), 0.0]
    pha = pha.astype(dtype).astype(np.float64)
    amp = amp.astype(dtype).astype(np.float64)
    return pha, amp, shifts, k["B"]


def min_gap(block, surr):
    """The smallest |v(s_i) - v(0)| per method over a case: [3]."""
    return np.abs(surr - block[..., :1]).reshape(-1, 3, surr.shape[-1]).transpose(1, 0, 2).reshape(3, -1).min(-1)
