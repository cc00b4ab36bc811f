"""Expected-gradients attributions with ``shap.GradientExplainer``'s call surface (the reference's
scripts/explain_fast.py / global_shap_analysis.py), and the band summary built on them.

For a model ``f: [*, C, T] -> [*, K]`` (eval-mode logits), a trial ``x_i``, background trials ``b_0 .. b_{M-1}`` and per
trial ``S`` draws ``(r_is, alpha_is)``::

    x'_is    = b_r + alpha_is (x_i - b_r)                        r = r_is
    phi_k[i] = (1/S) sum_s (x_i - b_r) * df_k/dx (x'_is)         [C, T] per trial and class

which is what ``shap``'s ``_PyTorchGradient.shap_values`` computes with ``local_smoothing = 0``.  ``shap``'s random
stream is not reproduced: the draws come from ``draw_samples`` (documented order, part of the interface).

The interpolation and the weighted, sequential sum are HIP kernels (``isd_attr_mix`` / ``isd_attr_accumulate``,
csrc/attr.hip); the gradients come from the model's own differentiable modules.  Pairs run in tiles of ``batch_size``
rows: device memory beyond the staged ``X`` and background is ``O(batch_size * C * T)`` plus one ``[n, C, T]``
accumulator per requested class.  Every class gets a forward pass of its own: the HIP modules' backward kernels work in
place on what the forward saved and release it, so a graph cannot be walked twice.
"""

import numpy as np
import torch

from . import _lib
from .constants import BANDS_5

__all__ = ["draw_samples", "GradientExplainer", "band_heatmap"]


def draw_samples(n, nsamples, n_background, rseed=0):
    """The draws of ``shap_values``: ``(ridx int32 [n, S] in [0, M), alpha float32 [n, S] in [0, 1))`` from
    ``rng = numpy.random.default_rng(rseed)`` as ``rng.integers(0, M, (n, S))`` followed by
    ``rng.random((n, S), dtype=float32)``."""
    n, S, M = int(n), int(nsamples), int(n_background)
    if n < 0 or S < 1 or M < 1:
        raise ValueError(f"draw_samples: need n >= 0, nsamples >= 1, n_background >= 1; got {n}, {S}, {M}")
    rng = np.random.default_rng(rseed)
    ridx = rng.integers(0, M, (n, S)).astype(np.int32)
    alpha = rng.random((n, S), dtype=np.float32)
    return ridx, alpha


def attr_mix(x, bg, ridx, alpha, out, pair0, n_pairs, S):
    """``isd_attr_mix`` on float32 CUDA ``x [n, E]``, ``bg [M, E]``, int32 ``ridx [n*S]``, float32 ``alpha [n*S]``:
    ``out[q] = bg[r] + alpha[p] (x[p // S] - bg[r])`` for the pairs ``p = pair0 + q``, ``q < n_pairs``."""
    E, M = x.shape[-1], bg.shape[0]
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().isd_attr_mix(x.data_ptr(), bg.data_ptr(), ridx.data_ptr(), alpha.data_ptr(),
                                           out.data_ptr(), int(n_pairs), int(pair0), int(S), E, M, _lib.stream()))
    return out


def attr_accumulate(x, bg, ridx, grad, acc, pair0, n_pairs, S, scale):
    """``isd_attr_accumulate``: ``acc[i] += (x[i] - bg[r]) * grad[q]`` in ``s`` order for the tile's pairs; a trial
    whose last pair is in the tile is multiplied by ``scale`` afterwards."""
    E, M = x.shape[-1], bg.shape[0]
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().isd_attr_accumulate(x.data_ptr(), bg.data_ptr(), ridx.data_ptr(), grad.data_ptr(),
                                                  acc.data_ptr(), int(n_pairs), int(pair0), int(S), E, M, float(scale),
                                                  _lib.stream()))
    return acc


def _as_f32(a, name):
    if isinstance(a, torch.Tensor):
        if a.dtype not in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
            raise TypeError(f"{name} must hold floating-point trials, got {a.dtype}")
        return a.detach()
    a = np.asarray(a)
    if a.dtype.kind != "f":
        raise TypeError(f"{name} must hold floating-point trials, got dtype {a.dtype}")
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32))


_COUNTERS = ("_calls", "_tail_calls")          # per-module dropout call counters (isd_amd.nn)


class GradientExplainer:
    """``shap.GradientExplainer(model, background)`` on the GPU.

    ``model``: a callable mapping a float32 CUDA ``[m, C, T]`` tensor that requires grad to logits ``[m, K]`` through
    modules that are differentiable with respect to their input (``nn.FAST``, ``FeatureCNN`` behind
    ``extract_features``, the registry heads, plain torch modules ...), or a fitted fp32 estimator
    (``FilterbankCNNClassifier``, ``FilterbankEEGNetClassifier``, ``FASTHeadClassifier``).  An ``nn.Module`` (and an
    estimator's network) is put in eval mode for the call and its training flags and dropout call counters are
    restored afterwards; any other callable is called as it is.  ``background``: ``[M, C, T]``, NumPy or tensor;
    staged on the device once, here."""

    def __init__(self, model, background, batch_size=256):
        if hasattr(model, "_differentiable_logits"):                # an estimator: refuses unfitted / bf16 here
            self._root, self._fn = model._differentiable_logits("explain")
            device = model._device()
        elif callable(model):
            self._root = model if isinstance(model, torch.nn.Module) else None
            self._fn = model
            device = None
        else:
            raise TypeError("model must be a callable [m, C, T] -> [m, K] or a fitted isd_amd estimator")
        if int(batch_size) < 1:
            raise ValueError(f"batch_size must be at least 1, got {batch_size}")
        self.batch_size = int(batch_size)
        bg = _as_f32(background, "background")
        if bg.dim() != 3 or bg.shape[0] < 1 or bg.shape[1] < 1 or bg.shape[2] < 1:
            raise ValueError(f"background must be [M, C, T] with M >= 1, got shape {tuple(bg.shape)}")
        if device is None:
            if bg.is_cuda:
                device = bg.device
            else:
                p = next(self._root.parameters(), None) if self._root is not None else None
                if p is not None and p.is_cuda:
                    device = p.device
                elif torch.cuda.is_available():
                    device = torch.device("cuda", torch.cuda.current_device())
                else:
                    raise RuntimeError("GradientExplainer needs an MI355X GPU: there is no CPU fallback")
        self.device = torch.device(device)
        self.background = bg.to(device=self.device, dtype=torch.float32).contiguous()

    # ------------------------------------------------------------------ the call
    def shap_values(self, X, nsamples=200, ranked_outputs=None, rseed=0, draws=None):
        """Expected gradients of every class, float32 NumPy ``[n, C, T, K]``; with ``ranked_outputs=R`` those of each
        trial's ``R`` largest logits at ``X`` as ``([n, C, T, R], ranks int64 [n, R])`` (descending, ties -> lowest
        index).  ``draws=(ridx, alpha)`` replaces ``draw_samples(n, nsamples, M, rseed)``.  Bitwise repeatable."""
        S = int(nsamples)
        if S < 1:
            raise ValueError(f"nsamples must be at least 1, got {nsamples}")
        M, Cc, T = self.background.shape
        Xd = _as_f32(X, "X")
        if Xd.dim() != 3 or tuple(Xd.shape[1:]) != (Cc, T):
            raise ValueError(f"X must be [n, {Cc}, {T}] like the background, got shape {tuple(Xd.shape)}")
        n, E = Xd.shape[0], Cc * T
        Xd = Xd.to(device=self.device, dtype=torch.float32).contiguous()
        ridx, alpha = self._draws(draws, n, S, M, rseed)
        flags = [] if self._root is None else [(m, m.training, {k: m.__dict__[k] for k in _COUNTERS if k in m.__dict__})
                                               for m in self._root.modules()]
        from .nn import AttentionBlock
        attn_calls = AttentionBlock._calls
        if self._root is not None:
            self._root.eval()
        try:
            with torch.cuda.device(self.device):
                return self._run(Xd, ridx, alpha, n, S, E, ranked_outputs)
        finally:
            for m, was, counters in flags:
                m.training = was
                m.__dict__.update(counters)
            AttentionBlock._calls = attn_calls

    def _draws(self, draws, n, S, M, rseed):
        if draws is None:
            ridx, alpha = draw_samples(n, S, M, rseed)
        else:
            ridx, alpha = (np.asarray(d.cpu() if isinstance(d, torch.Tensor) else d) for d in draws)
            if ridx.shape != (n, S) or alpha.shape != (n, S):
                raise ValueError(f"draws must be two [n, nsamples] = [{n}, {S}] arrays, got {ridx.shape}, {alpha.shape}")
            if ridx.dtype.kind not in "iu":
                raise TypeError(f"draws: ridx must hold integer background indices, got dtype {ridx.dtype}")
            if n and (int(ridx.min()) < 0 or int(ridx.max()) >= M):        # the kernels index bg with it unchecked
                raise ValueError(f"draws: ridx must lie in [0, {M})")
        ridx = torch.as_tensor(np.ascontiguousarray(ridx, dtype=np.int32)).to(self.device).reshape(-1)
        alpha = torch.as_tensor(np.ascontiguousarray(alpha, dtype=np.float32)).to(self.device).reshape(-1)
        return ridx, alpha

    def _logits(self, xin):
        out = self._fn(xin)
        if not isinstance(out, torch.Tensor) or out.dim() != 2 or out.shape[0] != xin.shape[0]:
            raise ValueError("the model must map [m, C, T] to logits [m, K]")
        if out.dtype != torch.float32 or out.grad_fn is None:
            raise TypeError("the model's logits must be float32 and differentiable with respect to its input")
        return out

    def _run(self, Xd, ridx, alpha, n, S, E, ranked_outputs):
        dev, bs = self.device, self.batch_size
        Cc, T = Xd.shape[1:]
        bg = self.background.view(-1, E)
        x2 = Xd.view(n, E)
        with torch.enable_grad():
            at_x = [self._logits(Xd[i:i + bs].detach().requires_grad_(True)).detach() for i in range(0, n, bs)]
        if n == 0:
            at_x = [self._logits(self.background[:1].detach().requires_grad_(True)).detach()[:0]]
        logits_x = torch.cat(at_x)
        K = logits_x.shape[1]
        if ranked_outputs is None:
            ranks, cols = None, torch.arange(K, device=dev)[None, :].expand(n, K)
        else:
            R = int(ranked_outputs)
            if not 1 <= R <= K:
                raise ValueError(f"ranked_outputs must lie in [1, {K}], got {ranked_outputs}")
            ranks = torch.sort(logits_x, dim=1, descending=True, stable=True)[1][:, :R]
            cols = ranks
        n_out = cols.shape[1]
        # the class of every pair's row, per requested column
        cls = [cols[:, j].repeat_interleave(S).contiguous() for j in range(n_out)]
        acc = torch.zeros((n_out, n, E), dtype=torch.float32, device=dev)
        n_pairs = n * S
        buf = torch.empty((min(bs, max(n_pairs, 1)), E), dtype=torch.float32, device=dev)
        for p0 in range(0, n_pairs, bs):
            m = min(bs, n_pairs - p0)
            attr_mix(x2, bg, ridx, alpha, buf, p0, m, S)
            for j in range(n_out):
                xin = buf[:m].view(m, Cc, T).detach().requires_grad_(True)
                with torch.enable_grad():
                    logits = self._logits(xin)
                    g, = torch.autograd.grad(logits.gather(1, cls[j][p0:p0 + m, None]).sum(), xin)
                if g.dtype != torch.float32:
                    raise TypeError(f"the model's input gradient must be float32, got {g.dtype}")
                attr_accumulate(x2, bg, ridx, g.contiguous(), acc[j], p0, m, S, 1.0 / S)
                del logits, g, xin
        phi = acc.view(n_out, n, Cc, T).permute(1, 2, 3, 0).contiguous().cpu().numpy()
        if ranks is None:
            return phi
        return phi, ranks.cpu().numpy().astype(np.int64)


def band_heatmap(phi_ct, sfreq, bands=BANDS_5, nperseg=64, noverlap=None):
    """The numbers behind global_shap_analysis.py:120-174: STFT of each channel's attribution trace (scipy-legacy
    defaults, ``noverlap = nperseg // 2``), mean magnitude over each band's inclusive bins.
    ``phi_ct``: ``[C, T]`` -> float32 NumPy ``[C, n_bands, J]``; ``[n, C, T]`` -> ``[n, C, n_bands, J]``.  NumPy or CUDA
    tensor in; runs ``Stft.bandpower(mode='magnitude', shared_signal=True)`` on the GPU."""
    from .features import Stft, band_bins
    a = _as_f32(phi_ct, "phi_ct")
    if a.dim() not in (2, 3):
        raise ValueError(f"phi_ct must be [C, T] or [n, C, T], got shape {tuple(a.shape)}")
    single = a.dim() == 2
    if not a.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("band_heatmap needs an MI355X GPU: there is no CPU fallback")
        a = a.cuda()
    a = a.to(torch.float32)
    y = (a[None] if single else a)[:, None].contiguous()                 # [n, 1, C, T]: one signal, every band
    st = Stft(y.shape[-1], nperseg, noverlap)
    bm = st.bandpower(y, band_bins(float(sfreq), st.nperseg, bands), mode="magnitude", shared_signal=True)
    out = bm.permute(0, 2, 1, 3).contiguous().cpu().numpy()              # [n, C, n_bands, J]
    return out[0] if single else out
