"""NumPy float64 restatement of ``Stft.bandpower`` (isd_stft_bandpower) on top of ``oracle.dsp.stft``, and the case
tables of test_bandpower_cpu.py and test_bandpower_gpu.py.

With Z [.., n/2 + 1, J] the scipy-legacy STFT of a row (periodic Hann, zero boundary, padded, 'spectrum' scaling), band
(klo, khi) of a row gives, per frame,

    power      P = mean over klo <= k <= khi of |Z_k|^2        magnitude  mean of |Z_k|        logpower  log(P + eps)

and 0 (before the log) for an empty band, khi < klo.  Per-band input y [B, nb, C, T] reduces band b of signal b;
``shared_signal`` reduces every band of the one signal y [B, 1, C, T].

The routes the call takes (csrc/stft.hip), and what ``isd_stft_bandpower_last_path`` reports for them:

    direct DFT   nperseg 64, hop 32, T <= 512, per-band input                                1 + 16 FULL
    block sums   hop 32 / 64, nperseg = 2^a hop with 4..64 blocks per frame, T <= 64 hop,
                 every band 1..6 interior bins, per-band input                               2 + 16 KB
    FFT          everything else                                                             3
"""
import functools

import numpy as np

from oracle import dsp as odsp

MODES = ("power", "magnitude", "logpower")
EPS = 1e-10
DIRECT, BLOCKSUM, FFT = 1, 2, 3


def band_power(y, nperseg, noverlap, bins, mode="logpower", eps=EPS, shared_signal=False):
    """y [B, nb or 1, C, T] -> (values [B, nb, C, J] float64 in ``mode``, raw power [B, nb, C, J] float64)."""
    y = np.asarray(y, dtype=np.float64)
    B, nbi, C, _ = y.shape
    assert nbi == (1 if shared_signal else len(bins))
    _, _, Z = odsp.stft(y, 1.0, nperseg, noverlap)                      # [B, nbi, C, n/2 + 1, J]
    J = Z.shape[-1]
    out = np.zeros((B, len(bins), C, J))
    power = np.zeros((B, len(bins), C, J))
    for b, (lo, hi) in enumerate(bins):
        if hi < lo:
            continue
        P = np.abs(Z[:, 0 if shared_signal else b, :, lo:hi + 1, :]) ** 2
        power[:, b] = P.mean(axis=-2)
        out[:, b] = np.sqrt(P).mean(axis=-2) if mode == "magnitude" else power[:, b]
    if mode == "logpower":
        out = np.log(out + eps)
    return out, power


def loud_mask(power):
    """The values the plain 1e-4 log-domain bound covers: power above the row's median over frames / 1e4."""
    return power > np.median(power, axis=-1, keepdims=True) / 1e4


def expected_path(nperseg, noverlap, T, bins, shared_signal=False):
    """The route of the table above as the reporter's family, with KB for the block sums (else 0)."""
    hop = nperseg - noverlap
    if shared_signal:
        return FFT, 0
    if nperseg == 64 and hop == 32 and T <= 512:
        return DIRECT, 0
    nblk = nperseg // hop
    if hop in (32, 64) and nperseg % hop == 0 and nblk in (4, 8, 16, 32, 64) and T <= 64 * hop and \
            all(1 <= hi - lo + 1 <= 6 and lo >= 1 and hi <= nperseg // 2 - 1 for lo, hi in bins):
        widest = max(hi - lo + 1 for lo, hi in bins)
        return BLOCKSUM, {1: 4, 2: 4, 3: 5, 4: 6, 5: 8, 6: 8}[widest]
    return FFT, 0


def scaled_bins(n):
    """The direct kernel's band set at nperseg n: DC, Nyquist, their neighbours, every bin, an empty band, a range
    and a single bin."""
    h = n // 2
    lo = max(1, 5 * h // 32)
    hi = min(h, max(lo + 1, 12 * h // 32))
    s = max(2, 13 * h // 32)
    return [(0, 0), (h, h), (1, 1), (h - 1, h - 1), (0, h), (1, 0), (lo, hi), (s, s)]


D8 = scaled_bins(64)            # (0,0) (32,32) (1,1) (31,31) (0,32) (1,0) (5,12) (13,13)
D9 = D8 + [(2, 3)]              # nine bands: a row count that is no multiple of 4

# name -> (T, B, C, bins); nperseg 64, noverlap 32.  J = 17 with the extra frame on lane 15 (512), a last frame that
# holds one sample under the window's zero (481, 33, 1), J = 16 (480), ragged rows (250), less than one chunk (31, 1).
DIRECT_CASES = {
    "t512_c1_full": (512, 2, 1, D8),         # 16 rows: FULL; every wave holds four bands
    "t512_c5_full": (512, 1, 5, D8),         # 40 rows: FULL; waves that mix two bands
    "t512_c3_ragged": (512, 1, 3, D9),       # 27 rows: not FULL, a last quad of three rows
    "t481_c3": (481, 2, 3, D8),
    "t480_c4": (480, 1, 4, D8),
    "t250_c5": (250, 2, 5, D8),
    "t33_c3": (33, 1, 3, D9),
    "t31_c1": (31, 2, 1, D8),
    "t1_c4": (1, 1, 4, D8),
}

# name -> (nperseg, noverlap, T, B, C, bins): one case per instance <hop, KB>, 4 / 8 / 16 / 64 blocks per frame, bands
# at bin 1 and at n/2 - 1 (their Hann neighbours are DC and Nyquist)
BLOCKSUM_CASES = {
    "h64_kb4": (256, 192, 4096, 2, 3, [(1, 1), (126, 127), (9, 10), (64, 64)]),          # T = 64 hop: J = 65
    "h64_kb5": (512, 448, 2052, 2, 3, [(1, 3), (253, 255), (40, 40), (100, 101)]),       # just above a whole pass
    "h64_kb6": (1024, 960, 1001, 2, 3, [(1, 4), (508, 511), (77, 77), (200, 202)]),      # ragged: scalar loads
    "h64_kb8": (4096, 4032, 50, 2, 3, [(1, 6), (2042, 2047), (300, 304), (1000, 1000)]),  # T < hop
    "h32_kb4": (2048, 2016, 2048, 2, 3, [(1, 2), (1022, 1023), (500, 500)]),             # T = 64 hop: J = 65
    "h32_kb5": (128, 96, 1030, 2, 3, [(1, 1), (61, 63), (30, 32)]),                      # above a pass, T % 4 != 0
    "h32_kb6": (256, 224, 20, 2, 3, [(1, 4), (124, 127), (60, 60)]),                     # T < hop
    "h32_kb8": (512, 480, 777, 2, 3, [(1, 5), (250, 255), (100, 100)]),                  # ragged; 5- and 6-bin bands
    "h64_kb8_j65": (4096, 4032, 4096, 1, 2, [(1, 6), (2046, 2047)]),                     # 64 blocks per frame, J = 65
    "h64_single_bins": (1024, 960, 1500, 2, 3, [(1, 1), (511, 511), (17, 17)]),          # unused slots repeat a row
    "h32_single_bins": (512, 480, 2047, 2, 3, [(1, 1), (255, 255), (128, 128)]),
}


def _swap(bins, i, band):
    out = list(bins)
    out[i] = band
    return out


# the same plans with one band the block sums do not take: seven bins, DC, Nyquist -> the FFT kernel
def _fallbacks():
    out = {}
    for base, kinds in [("h64_kb4", ("wide", "dc", "nyq")), ("h64_kb6", ("wide",)), ("h32_kb4", ("dc",)),
                        ("h32_kb8", ("nyq",)), ("h64_kb8_j65", ("wide",))]:
        n, nov, T, B, C, bins = BLOCKSUM_CASES[base]
        for kind in kinds:
            band = {"wide": (n // 4, n // 4 + 6), "dc": (0, 2), "nyq": (n // 2 - 1, n // 2)}[kind]
            out[f"{base}_{kind}"] = (n, nov, T, B, C, _swap(bins, 1, band))
    return out


FALLBACK_CASES = _fallbacks()

# 64 bands at nperseg 8: every (lo, hi) with 0 <= lo, hi <= 4 -- ten of the 25 empty -- repeated
B64 = [(lo, hi) for lo in range(5) for hi in range(5)] * 3
B64 = B64[:64]

# name -> (nperseg, noverlap, T, B, C, bins); hops that do not divide nperseg, frame counts that leave dead frames in
# the last workgroup (256 / min(nperseg / 2, 256) frames each), and the direct kernel's upper edge (64 / 32, T > 512)
FFT_CASES = {
    "n8": (8, 0, 37, 1, 3, scaled_bins(8)),                       # 64 frames per workgroup; 144 / 18 frames
    "n8_64bands": (8, 0, 37, 1, 3, B64),                          # more bands than the 4 threads of a frame
    "n32": (32, 9, 120, 1, 3, scaled_bins(32)),                   # 16 per workgroup; 168 / 21 frames
    "n128": (128, 100, 310, 1, 3, scaled_bins(128) + [(2, 3)]),   # 4 per workgroup; 351 / 39 frames
    "n512": (512, 300, 1000, 1, 3, scaled_bins(512)),             # one frame per workgroup
    "n2048": (2048, 1024, 3000, 1, 2, scaled_bins(2048)),
    "n64_t513": (64, 32, 513, 1, 3, D8),                          # a last frame under the window's zero
    "n64_t800": (64, 32, 800, 1, 3, D9),
}


def all_cases():
    """(table name, case name, nperseg, noverlap, T, B, C, bins, shared_signal) of every band-power case."""
    for name, (T, B, C, bins) in DIRECT_CASES.items():
        yield "direct", name, 64, 32, T, B, C, bins, False
    for table, cases in (("blocksum", BLOCKSUM_CASES), ("fallback", FALLBACK_CASES)):
        for name, (n, nov, T, B, C, bins) in cases.items():
            yield table, name, n, nov, T, B, C, bins, False
    for name, (n, nov, T, B, C, bins) in FFT_CASES.items():
        yield "fft", name, n, nov, T, B, C, bins, False
        yield "fft", name + "_shared", n, nov, T, B, C, bins, True


CASES = {f"{c[0]}-{c[1]}": c[2:] for c in all_cases()}


def case_names(table):
    return [k for k in CASES if k.startswith(table + "-")]


def plans():
    """Every distinct (T, nperseg, noverlap) of the tables."""
    return sorted({(T, n, nov) for n, nov, T, *_ in CASES.values()})


@functools.lru_cache(maxsize=None)
def make(case):
    """The fp32 standard-normal rows of a case, seeded by its name: [B, nb or 1, C, T]."""
    n, nov, T, B, C, bins, shared = CASES[case]
    seed = int.from_bytes(case.encode(), "little") % (2 ** 32)
    y = np.random.default_rng(seed).standard_normal((B, 1 if shared else len(bins), C, T)).astype(np.float32)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def reference(case):
    """{mode: values} and the raw power of a case, computed once and shared (read-only)."""
    n, nov, T, B, C, bins, shared = CASES[case]
    out = {}
    for mode in MODES:
        out[mode], power = band_power(make(case), n, nov, bins, mode, EPS, shared)
        out[mode].setflags(write=False)
    power.setflags(write=False)
    return out, power
