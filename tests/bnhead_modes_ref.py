"""Cases, parameter randomiser and fp64 runner for the BatchNorm heads' eval mode, running statistics and input
gradients: EEGNet_Encoder, CVBlock (csrc/eegnet.hip) and HeadConv_Paper_Version (csrc/paperhead.hip), driven from
isd_amd/nn.py.  Shared by test_bnheads_modes_cpu.py, which shows on the reference alone that every case is well
conditioned and that the running-variance cases see BatchNorm's N / (N - 1) factor, and test_bnheads_modes_gpu.py, which
holds the kernels to the reference.

Every case is the smallest shape that reaches the route named beside it.  Trials and cotangent are unit-scale
``torch.randn`` seeded per case and dropout is 0: the comparison is about the kernels' logic, not their conditioning.

The bounds are those of tests/test_eegnet_gpu.py::test_bn_heads_input_gradient_vs_oracle (output 1e-4, input gradient
2e-4, each parameter gradient 2e-4 of the largest gradient magnitude over all parameters) and of the golden tests
(running statistics 1e-4; ``running_var`` is held element by element here)."""
import contextlib
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cnn as ocnn

OUT_TOL, XGRAD_TOL, PGRAD_TOL, RUNNING_TOL = 1e-4, 2e-4, 2e-4, 1e-4
DEFAULT_HYPER = (0.1, 1e-5)            # nn.BatchNorm2d's momentum and eps
TRAIN_HYPER = (0.3, 1e-3)              # the train step's non-default pair
VAR_MOMENTUM = 0.5                     # of the running-variance cases
VAR_MARGIN = 50.0                      # a biased variance misses a running-variance case's bound by this factor


class Case(NamedTuple):
    kind: str           # "eegnet" / "cvblock" / "paper"
    C: int
    T: int
    K: int              # kernel_length (EEGNet only; 0 elsewhere)
    B: int
    F: int = 16
    reseed: int = 0     # moved when a draw turns out badly conditioned (test_bnheads_modes_cpu.py decides)

    @property
    def seed(self):
        return 1000003 * self.reseed + 7919 * self.C + 31 * self.T + 7 * self.K + self.B + self.F

    @property
    def id(self):
        k = f"-K{self.K}" if self.kind == "eegnet" else ""
        return f"{self.kind}-C{self.C}-T{self.T}{k}-B{self.B}-F{self.F}"


def _eeg(C, T, K, B):
    return Case("eegnet", C, T, K, B)


def _cv(C, T, B):
    return Case("cvblock", C, T, 0, B)


def _paper(C, T, B, Fd, reseed=0):
    return Case("paper", C, T, 0, B, Fd, reseed)


EEGNET_CASES = [
    _eeg(3, 27, 6, 2),        # shortest row the pooling allows; Gram statistics with MT = 2; runtime-K instances
    _eeg(5, 47, 16, 3),       # MT = 3; the <16> instances
    _eeg(4, 63, 32, 2),       # the MT 4 / 5 boundary ...
    _eeg(4, 64, 32, 2),       # ... and its other side
    _eeg(3, 79, 64, 2),       # last row length of the Gram statistics ...
    _eeg(3, 80, 64, 2),       # ... first of the bulk + edge statistics
    _eeg(130, 47, 32, 2),     # wide rows kernel (C >= 128) with the Gram statistics
    _eeg(129, 161, 64, 2),    # wide rows kernel; 11 column tiles in groups of 5
    _eeg(2, 1030, 64, 2),     # two segments of eeg_bwd_corr_kernel; five of eeg_bwd_dx_kernel
    _eeg(2, 257, 48, 2),      # one sample into the second dx segment; runtime K
    _eeg(260, 40, 16, 2),     # second channel block of eeg_bwd_dws_kernel; dx grid of B * C rows
    _eeg(2, 27, 64, 70),      # B * 16 = 1120 rows: second round of the row loops and of eeg_bwd3_sums_kernel
]
CVBLOCK_T_RANGE = (247, 262)   # the window lengths whose pooled width is the projector's 256 (fast.py:66-74)
CVBLOCK_CASES = [
    _cv(4, 247, 3),           # shortest window the projector takes
    _cv(10, 262, 70),         # longest; B * 16 > 1024 rows
    _cv(130, 250, 2),         # the wide rows kernel under CVBlock
]
PAPER_CASES = [
    _paper(1, 46, 3, 3),      # every minimum: one channel, layer widths 1 / 1 / 1 / 3, one step left after the last pool
    _paper(5, 47, 4, 64),     # widest layers, 32 / 21 / 21 / 64; odd lengths at layer 1
    _paper(33, 46, 3, 49),    # layer widths 24 / 16 / 16 / 49; three input-channel tiles, the last ragged
    # B * To = 545 600 > 2048 * 256 (conv clamp); 2 to 3 trials per wgrad slab; pool clamp.  Over half a million
    # max-pool pairs: most draws hold one that fp32 decides the other way (the conditions of test_bnheads_modes_cpu.py
    # refuse them: of the reseeds 0 .. 39 they leave 9, 19, 23 and 38; 19 has the widest margin)
    _paper(2, 250, 2200, 3, reseed=19),
]
CASES = EEGNET_CASES + CVBLOCK_CASES + PAPER_CASES
FIRST_OF_EACH_HEAD = [EEGNET_CASES[0], CVBLOCK_CASES[0], PAPER_CASES[0]]

# Batches small enough that the N / (N - 1) factor of running_var is far above the bound (forward and buffers only:
# they are degenerate for BatchNorm's backward).  Momentum VAR_MOMENTUM.
VAR_CASES = [_eeg(1, 27, 6, 1), _eeg(2, 40, 16, 1), _paper(1, 46, 1, 3), _paper(3, 50, 2, 6), _cv(1, 250, 1)]


def make_module(inn, case):
    if case.kind == "eegnet":
        return inn.EEGNet_Encoder(case.C, case.F, kernel_length=case.K, dropout=0.0)
    if case.kind == "cvblock":
        return inn.CVBlock(case.C, case.F, dropout=0.0)
    return inn.HeadConv_Paper_Version(case.C, case.F)


def randomise_bn(m):
    """BatchNorm affine parameters away from (1, 0) and running statistics away from (0, 1)."""
    with torch.no_grad():
        for bn in m._bns():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.3, 0.3)
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 2.0)


def build_case(inn, case):
    """-> (module on the CPU in its initial state, x [B, C, T], w [B, F]); the same on every machine."""
    torch.manual_seed(case.seed)
    m = make_module(inn, case)
    randomise_bn(m)
    return m, torch.randn(case.B, case.C, case.T), torch.randn(case.B, case.F)


def set_hyper(m, momentum, eps):
    for bn in m._bns():
        bn.momentum, bn.eps = momentum, eps


def ref_params(m, dtype=torch.float64):
    """The module's state as CPU leaves of ``dtype`` keyed like its state_dict; parameters ask for gradients."""
    p = {}
    for k, v in m.state_dict().items():
        v = v.detach().cpu().clone()
        p[k] = v if "num_batches" in k else v.to(dtype)
        if "running" not in k and "num_batches" not in k:
            p[k].requires_grad_()
    return p


class _BiasedF:
    """``torch.nn.functional`` with a train-mode ``batch_norm`` that feeds the BIASED batch variance into
    ``running_var``: what a kernel without the N / (N - 1) factor would leave behind."""

    def __getattr__(self, name):
        return getattr(F, name)

    @staticmethod
    def batch_norm(h, running_mean, running_var, weight, bias, training, momentum, eps):
        if not training:
            return F.batch_norm(h, running_mean, running_var, weight, bias, False, momentum, eps)
        with torch.no_grad():
            dims = [d for d in range(h.dim()) if d != 1]
            running_mean.mul_(1 - momentum).add_(momentum * h.mean(dims))
            running_var.mul_(1 - momentum).add_(momentum * h.var(dims, unbiased=False))
        return F.batch_norm(h, None, None, weight, bias, True, momentum, eps)


POOL_JITTER = 4.0 * 2.0 ** -23        # four fp32 ulps of each max-pool input


class _JitterPoolF:
    """``torch.nn.functional`` with a ``max_pool2d`` that DECIDES on its input times (1 + POOL_JITTER * N(0, 1)) and
    routes the unperturbed values: the pairs an fp32 implementation may decide either way, decided at random."""

    def __init__(self, seed):
        self.gen = torch.Generator().manual_seed(seed)

    def __getattr__(self, name):
        return getattr(F, name)

    def max_pool2d(self, h, kernel, stride):
        assert tuple(kernel) == (1, 2) and tuple(stride) == (1, 2)
        noisy = h.detach() * (1 + POOL_JITTER * torch.randn(h.shape, generator=self.gen, dtype=h.dtype))
        _, idx = F.max_pool2d(noisy, kernel, stride=stride, return_indices=True)
        return h.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)


@contextlib.contextmanager
def _oracle_functional(f):
    saved, ocnn.F = ocnn.F, f
    try:
        yield
    finally:
        ocnn.F = saved


def oracle_forward(case, x, p, training, momentum, eps):
    if case.kind == "eegnet":
        return ocnn.eegnet_encoder(x, p, training=training, momentum=momentum, eps=eps, kernel_length=case.K)
    if case.kind == "cvblock":
        return ocnn.cvblock(x, p, training=training, momentum=momentum, eps=eps)
    return ocnn.headconv_paper(x, p, training=training, momentum=momentum, eps=eps)


def run_reference(case, m, x, w, training, momentum=DEFAULT_HYPER[0], eps=DEFAULT_HYPER[1], dtype=torch.float64,
                  grads=True, biased_var=False, pool_jitter=None):
    """One pass of the oracle from the state of ``m`` (left untouched) in ``dtype``.  -> dict(y, x_grad, grads
    {name: tensor}, buffers {name: tensor after the pass}); without ``grads`` the pass is forward only.
    ``biased_var`` / ``pool_jitter`` (a seed): the defective / perturbed variants of the classes above."""
    functional = _BiasedF() if biased_var else F if pool_jitter is None else _JitterPoolF(pool_jitter)
    p = ref_params(m, dtype)
    xr = x.detach().cpu().to(dtype).requires_grad_(grads)
    with _oracle_functional(functional), torch.set_grad_enabled(grads):
        y = oracle_forward(case, xr, p, training, momentum, eps)
        if grads:
            (y * w.detach().cpu().to(dtype)).sum().backward()
    return {"y": y.detach(), "x_grad": xr.grad,
            "grads": {k: v.grad for k, v in p.items() if v.grad is not None},
            "buffers": {k: v.detach() for k, v in p.items() if "running" in k}}


# ----------------------------------------------------------------------------- the comparison's metrics
def _f64(t):
    return np.asarray(t.detach().cpu().double().numpy() if torch.is_tensor(t) else t, dtype=np.float64)


def rel(got, want):
    """conftest.rel_err: largest deviation over the reference's largest magnitude."""
    got, want = _f64(got), _f64(want)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def elementwise_rel(got, want):
    """Largest |got - want| / want, element by element (``running_var``: every element is positive)."""
    got, want = _f64(got), _f64(want)
    return float((np.abs(got - want) / want).max())


def grad_scale(want_grads):
    return max(float(g.abs().max()) for g in want_grads.values())


def var_bounds(want, biased):
    """{name: bound} on the ``running_var`` buffers of a running-variance case.  ``biased``: the pass recomputed with
    the biased variance.  That defect moves an element of a layer with N values per channel by
    momentum * v / (N - 1) / running_var < 1 / (N - 1), and by much less where the layer's batch variance v is small
    against the randomised running_var, so no input makes every element of every layer move by VAR_MARGIN times
    RUNNING_TOL (CVBlock's first two layers have N >= 248).  Each layer is therefore held to the smaller of RUNNING_TOL
    and 1 / VAR_MARGIN of the largest move among its elements: a biased variance in any one layer misses that layer's
    bound by the margin."""
    out = {}
    for k, v in want["buffers"].items():
        if k.endswith("running_var"):
            out[k] = min(RUNNING_TOL, elementwise_rel(biased["buffers"][k], v) / VAR_MARGIN)
    return out


def errors(got, want, gradients=True, buffers=True, bounds=None):
    """{quantity: (error, bound)} of one pass against the reference, each in its own metric.  ``got``: dict like
    ``run_reference``'s (``grads`` / ``buffers`` keyed by state_dict names).  ``bounds``: {buffer name: bound} that
    replace RUNNING_TOL (``var_bounds``)."""
    out = {"y": (rel(got["y"], want["y"]), OUT_TOL)}
    if gradients:
        out["x_grad"] = (rel(got["x_grad"], want["x_grad"]), XGRAD_TOL)
        scale = grad_scale(want["grads"])
        assert set(got["grads"]) == set(want["grads"])
        for k, g in want["grads"].items():
            out["grad " + k] = (float(np.abs(_f64(got["grads"][k]) - _f64(g)).max()) / scale, PGRAD_TOL)
    if buffers:
        assert set(got["buffers"]) == set(want["buffers"])
        for k, v in want["buffers"].items():
            metric = elementwise_rel if k.endswith("running_var") else rel
            out[k] = (metric(got["buffers"][k], v), (bounds or {}).get(k, RUNNING_TOL))
    return out


def quantity_class(name):
    """The row of the recorded-error table a quantity of ``errors`` belongs to."""
    if name.startswith("grad "):
        return "parameter gradients"
    return {"y": "output", "x_grad": "input gradient"}.get(name, name.rsplit(".", 1)[-1])
