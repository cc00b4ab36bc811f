"""NumPy complex128 restatement of isd_amd/tfr.py, written from the documented behaviour of
mne.time_frequency.morlet / cwt / tfr_array_morlet and independent of the package: the wavelet formula written out
again, one np.convolve(row, W, 'same')[::decim] per (row, frequency), the six outputs from the complex map.  In
'itc' a sample with |z| = 0 contributes 0.  Shared by test_tfr_cpu.py and test_tfr_gpu.py.

CASES is shared too: (data shape, sfreq, freqs, n_cycles)."""
import numpy as np

F_B = np.arange(8.0, 41.0, 2.0)                                    # 17 frequencies
F_G = np.linspace(20.0, 100.0, 17)
CASES = {
    "A": ((3, 2, 96), 250.0, np.array([20.0, 31.0, 40.0, 60.0, 100.0]), 3.0),   # T below one tile; 11 .. 59 taps
    "B": ((2, 3, 300), 250.0, F_B, F_B / 2.0),                     # 17 frequencies of 199 taps each
    "C": ((1, 1, 697), 250.0, np.array([4.0]), 7.0),               # taps == T: zero-fill on both sides of every output
    "D": ((2, 2, 795), 250.0, np.array([4.0, 5.0, 39.0, 40.0]), 7.0),      # 697 and 69 taps in one call
    "E": ((1, 2, 4200), 1024.0, np.array([2.8, 100.0]), 7.0),      # 4075 taps; T beyond one tile with a remainder
    "F": ((5, 2, 2500), 250.0, np.array([10.0, 40.0]), 7.0),       # several time tiles; five trials
    # three frequency groups on enough (channel, tile) pairs that the averaged kernels keep their 512-output tile:
    # four chunks per tile, one group per workgroup, blockIdx.y = 0 .. 2
    "G": ((2, 32, 3000), 250.0, F_G, 2.0),                         # 41 .. 9 taps
}


def make_data(shape, sfreq, seed=0):
    """standard_normal + 2 sin(2 pi 10 t) + a per-trial offset cycling through 0, 50, -200 (float64)."""
    rng = np.random.default_rng(seed + int(np.prod(shape)))
    n, C, T = shape
    x = rng.standard_normal(shape) + 2.0 * np.sin(2.0 * np.pi * 10.0 * np.arange(T) / sfreq)
    x += np.array([0.0, 50.0, -200.0])[np.arange(n) % 3][:, None, None]
    return x


def morlet(sfreq, freqs, n_cycles=7.0, sigma=None, zero_mean=False):
    freqs = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    n_cycles = np.broadcast_to(np.asarray(n_cycles, dtype=np.float64), freqs.shape)
    out = []
    for k in range(freqs.size):
        f = freqs[k]
        sigma_t = n_cycles[k] / (2.0 * np.pi * f) if sigma is None else n_cycles[k] / (2.0 * np.pi * sigma)
        half = np.arange(0.0, 5.0 * sigma_t, 1.0 / sfreq)
        t = np.concatenate([-half[::-1], half[1:]])
        carrier = np.cos(2.0 * np.pi * f * t) + 1j * np.sin(2.0 * np.pi * f * t)
        if zero_mean:
            carrier = carrier - np.exp(-2.0 * (np.pi * f * sigma_t) ** 2)
        W = carrier * np.exp(-(t * t) / (2.0 * sigma_t * sigma_t))
        W = W / (np.sqrt(0.5) * np.sqrt(np.sum(np.abs(W) ** 2)))
        out.append(W)
    return out


def cwt(X, Ws, decim=1):
    """X [rows, T] -> complex128 [rows, F, ceil(T / decim)]."""
    X = np.asarray(X, dtype=np.float64)
    rows, T = X.shape
    out = np.empty((rows, len(Ws), -(-T // decim)), dtype=np.complex128)
    for r in range(rows):
        for j, W in enumerate(Ws):
            assert len(W) % 2 == 1 and len(W) <= T
            out[r, j] = np.convolve(X[r], W, "same")[::decim]
    return out


def outputs(z):
    """The six outputs from the complex map z [n, C, F, T_out]."""
    mag = np.abs(z)
    unit = np.divide(z, mag, out=np.zeros_like(z), where=mag > 0)
    power = z.real ** 2 + z.imag ** 2
    avg, itc = power.mean(0), np.abs(unit.mean(0))
    return {"complex": z, "power": power, "phase": np.angle(z), "avg_power": avg, "itc": itc,
            "avg_power_itc": avg + 1j * itc}


def tfr(data, sfreq, freqs, n_cycles=7.0, zero_mean=True, decim=1):
    """data [n, C, T] -> the dict of the six outputs."""
    data = np.asarray(data, dtype=np.float64)
    n, C, T = data.shape
    Ws = morlet(sfreq, freqs, n_cycles, zero_mean=zero_mean)
    z = cwt(data.reshape(n * C, T), Ws, decim).reshape(n, C, len(Ws), -1)
    return outputs(z)
