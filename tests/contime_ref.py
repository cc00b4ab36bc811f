"""NumPy float64 restatement of isd_amd.connectivity.spectral_connectivity_time, straight from the table of its
docstring and independent of the package.  With s = w_i conj(w_j), u = s / |s| (0 where |s| = 0) and <.> the mean
over the samples t0 <= t < t1:

    coh    |<s>| / sqrt(<|w_i|^2> <|w_j|^2>)        pli    |<sign Im s>|
    imcoh  Im <s> / sqrt(<|w_i|^2> <|w_j|^2>)       dpli   <H(Im s)>, H(0) = 1/2
    plv    |<u>|                                    wpli   |<Im s>| / <|Im s|>
    ciplv  |Im <u>| / sqrt((1 - |Re <u>|)(1 + |Re <u>|))
    wpli2_debiased  ((sum Im s)^2 - sum (Im s)^2) / ((sum |Im s|)^2 - sum (Im s)^2)

``ref_contime`` works on a given complex map and broadcasts one [n, F, C, C, T] array; every entry, the diagonal
included, is what the formula gives (0 / 0 = NaN).  ``ref_spectral_connectivity_time`` composes it with the transform
of tfr_ref.  Shared by test_contime_cpu.py and test_contime_gpu.py, with the case table and ``make``."""
import numpy as np

import tfr_ref

METHODS = ("coh", "imcoh", "plv", "ciplv", "pli", "dpli", "wpli", "wpli2_debiased")
SIGN_BASED = ("pli", "dpli")
ANTISYMMETRIC = ("imcoh", "dpli")
# what the package sets on the diagonal (it does not compute it)
DIAGONAL = {"coh": 1.0, "plv": 1.0, "imcoh": 0.0, "pli": 0.0, "dpli": 0.5, "ciplv": np.nan, "wpli": np.nan,
            "wpli2_debiased": np.nan}
# a dead channel against a live one
DEAD = {"coh": np.nan, "imcoh": np.nan, "wpli": np.nan, "wpli2_debiased": np.nan, "plv": 0.0, "ciplv": 0.0,
        "pli": 0.0, "dpli": 0.5}

CASES = {                            # name -> (n, C, F, T)
    "one": (1, 1, 1, 5),             # the smallest shape
    "tiles": (2, 20, 3, 70),         # two channel tiles, a ragged second, several time chunks with a tail, F > 1
    "wide": (1, 33, 2, 37),          # three tiles, one channel in the last
    "c128": (1, 128, 1, 19),         # the channel limit, all 36 tile pairs
}


def make(case):
    """The complex64 map [n, C, F, T] of a case."""
    shape = CASES[case]
    r = np.random.default_rng(0)
    return (r.standard_normal(shape) + 1j * r.standard_normal(shape)).astype(np.complex64)


def cross(z, t0, t1):
    """s [n, F, C, C, T'] = w_i conj(w_j) of z [n, C, F, T] over t0 <= t < t1, in complex128."""
    w = np.asarray(z, dtype=np.complex128)[..., t0:t1].transpose(0, 2, 1, 3)          # [n, F, C, T']
    return w[:, :, :, None, :] * np.conj(w[:, :, None, :, :])


def ref_contime(z, methods, t0, t1):
    """z complex [n, C, F, T] -> {method: float64 [n, F, C, C]}."""
    s = cross(z, t0, t1)
    w = np.asarray(z, dtype=np.complex128)[..., t0:t1].transpose(0, 2, 1, 3)
    p = (np.abs(w) ** 2).mean(-1)                                                    # [n, F, C]
    mag = np.abs(s)
    u = np.divide(s, mag, out=np.zeros_like(s), where=mag > 0)
    im = s.imag
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.sqrt(p[:, :, :, None] * p[:, :, None, :])
        for m in methods:
            if m == "coh":
                v = np.abs(s.mean(-1)) / den
            elif m == "imcoh":
                v = s.mean(-1).imag / den
            elif m == "plv":
                v = np.abs(u.mean(-1))
            elif m == "ciplv":
                e = u.mean(-1)
                v = np.abs(e.imag) / np.sqrt((1.0 - np.abs(e.real)) * (1.0 + np.abs(e.real)))
            elif m == "pli":
                v = np.abs(np.sign(im).mean(-1))
            elif m == "dpli":
                v = np.where(im > 0, 1.0, np.where(im < 0, 0.0, 0.5)).mean(-1)
            elif m == "wpli":
                v = np.abs(im.mean(-1)) / np.abs(im).mean(-1)
            elif m == "wpli2_debiased":
                sq = (im * im).sum(-1)
                v = (im.sum(-1) ** 2 - sq) / (np.abs(im).sum(-1) ** 2 - sq)
            else:
                raise ValueError(m)
            out[m] = v
    return out


def sign_margin(z, t0, t1):
    """The smallest |Im s| / (|w_i| |w_j|) over the off-diagonal pairs and the samples (inf for one channel)."""
    s = cross(z, t0, t1)
    C = s.shape[2]
    if C < 2:
        return np.inf
    off = ~np.eye(C, dtype=bool)
    return float((np.abs(s.imag) / np.abs(s))[:, :, off].min())


def ref_spectral_connectivity_time(data, freqs, methods, sfreq, n_cycles=7.0, decim=1, zero_mean=True, padding=0.0):
    """data real [n, C, T] -> ({method: [n, F, C, C]}, the complex map, t0, t1)."""
    z = tfr_ref.tfr(data, sfreq, freqs, n_cycles, zero_mean=zero_mean, decim=decim)["complex"]
    t0 = int(round(padding * sfreq / decim))
    t1 = z.shape[-1] - t0
    return ref_contime(z, methods, t0, t1), z, t0, t1
