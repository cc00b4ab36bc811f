"""The analytic signal and the amplitude envelope on the GPU: the amplitude side of the signal toolbox, next to the
phase and coherence measures of ``connectivity``.

``hilbert(x, N=None)`` is ``scipy.signal.hilbert(x, N, axis=-1)``: the FFT of x (zero-padded or cut to N samples,
default T), times the one-sided weights h (1 at DC, 1 at Nyquist for even N, 2 between, 0 above), inverse FFT; the
result is complex of length N.  MNE's ``apply_hilbert(n_fft=F)`` is ``hilbert(x, F)[..., :T]``.

``envelope(x, N=None)`` is ``abs(hilbert(x, N))[..., :T]``, real.

Both run as ``torch.fft.fft`` -> weights -> ``torch.fft.ifft`` on the device.  This is plumbing, O(T log T) per row;
the data-sized consumer of the analytic signal is the pair kernel behind ``connectivity.envelope_correlation``,
O(C T) per row (csrc/envcorr.hip).  There is no CPU fallback.  ndarray in -> computed in fp64 on the GPU -> complex128
/ float64 ndarray out; float32 / float64 CUDA tensor in -> CUDA tensor of the matching complex / real dtype out; a CPU
tensor or a non-float dtype raises TypeError.  Importing this module touches neither the GPU nor the library.
"""

import numpy as np
import torch

from . import _lib


def _check(x, N):
    """-> (x, is_tensor, N): every check that needs no GPU."""
    x, is_tensor = _lib.check_array(x, "x")
    if x.ndim < 1 or x.shape[-1] < 1:
        raise ValueError(f"x must have at least one sample along its last axis, got {tuple(x.shape)}")
    if N is None:
        N = int(x.shape[-1])
    elif isinstance(N, bool) or int(N) != N or int(N) < 1:
        raise ValueError(f"N={N!r} must be a positive integer")
    return x, is_tensor, int(N)


def analytic_weights(N, dtype, device):
    """The one-sided weights of scipy.signal.hilbert, [N] real on ``device``."""
    h = torch.zeros(N, dtype=dtype, device=device)
    h[0] = 1
    if N % 2 == 0:
        h[N // 2] = 1
        h[1:N // 2] = 2
    else:
        h[1:(N + 1) // 2] = 2
    return h


def hilbert_device(xd, N):
    """x on the device, real [..., T] -> complex [..., N]."""
    X = torch.fft.fft(xd, n=N, dim=-1)
    return torch.fft.ifft(X * analytic_weights(N, xd.dtype, xd.device), dim=-1)


def hilbert(x, N=None):
    """The analytic signal of real x along its last axis, complex [..., N] (N defaults to T): the arguments and the
    result of ``scipy.signal.hilbert(x, N, axis=-1)``; ``mne.apply_hilbert(n_fft=F)`` is ``hilbert(x, F)[..., :T]``.
    ``torch.fft`` on the device, O(T log T) per row, against the O(C T) per row of the pair kernel that consumes it
    in ``connectivity.envelope_correlation``."""
    x, is_tensor, N = _check(x, N)
    z = hilbert_device(_lib.to_device(x, is_tensor, "hilbert"), N)
    return z if is_tensor else z.cpu().numpy()


def envelope(x, N=None):
    """``abs(hilbert(x, N))[..., :T]``: the amplitude envelope of real x, real."""
    x, is_tensor, N = _check(x, N)
    T = int(x.shape[-1])
    e = hilbert_device(_lib.to_device(x, is_tensor, "envelope"), N).abs()[..., :T]
    return e if is_tensor else e.cpu().numpy()
