"""Host restatement of the train-mode dropout of the BatchNorm heads EEGNet_Encoder and CVBlock (csrc/eegnet.hip, driven
from isd_amd/nn.py): the two counter-based keep-masks of a call, and the oracle's networks (oracle/cnn.py:76-119) in
the dtype of their arguments with the masks multiplied in after each of the two average pools.

The kernels evaluate ``drop_scale(stream, idx, p)`` -- the hash of ``tail_ref.drop_keep_mask`` -- per element:

* site 1, after the first pool: stream ``s1 = seed + 0xD1342543DE82EF95 * counter`` (mod 2^64), element [b, g, v] of
  [B, 16, T2] at flat index (b * 16 + g) * T2 + v;
* site 2, after the second pool: stream ``s1 ^ 0x5bd1e995``, element [b, h, v] of [B, 16, T3] at (b * 16 + h) * T3 + v.

``seed`` is ``nn._dropout_seed(m._stream_id, m._calls)`` read after the forward (the call counter moves before it is
used); ``counter`` is the device-resident step counter of ``set_seed_counter`` (0 without one).  A kept element is
multiplied by the fp32 value 1 / (1 - p).

The module also holds the cases of test_bnheads_dropout_gpu.py, with everything that fixes their masks (torch seed,
stream id), so that test_bnheads_dropout_cpu.py can show on the reference alone that each of them tells a wrong mask
from the right one.  Shared by those two files."""
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cnn as ocnn
from tail_ref import drop_keep_mask

M64 = (1 << 64) - 1
COUNTER_STEP = 0xD1342543DE82EF95
SITE2_XOR = 0x5bd1e995


def geometry(kind, T, kernel_length=64):
    """(T2, T3) of the plan: the widths the two dropout sites see (eeg_plan_create in csrc/eegnet.hip)."""
    P1, P2 = (4, 8) if kind == "eegnet" else (8, 2)
    K = kernel_length if kind == "eegnet" else 64
    Tp = T + 2 * (K // 2) - K + 1
    T2 = Tp // P1
    T2p = T2 + 1
    return T2, T2p // P2


def site_streams(seed, counter=0):
    """The two sites' hash streams of one call."""
    s1 = (int(seed) + COUNTER_STEP * int(counter)) & M64
    return s1, s1 ^ SITE2_XOR


def head_masks(kind, seed, counter, B, T, kernel_length, p):
    """-> (mask1 [B, 16, T2], mask2 [B, 16, T3]), fp64 tensors of 0 / 1 (1: kept)."""
    T2, T3 = geometry(kind, T, kernel_length)
    s1, s2 = site_streams(seed, counter)
    return drop_keep_mask(s1, (B, 16, T2), p), drop_keep_mask(s2, (B, 16, T3), p)


def keep_scale(drop_p):
    """1 / (1 - p) as the kernel forms it: in fp32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(drop_p)))


def _drop(h, mask, scale):
    return h * mask.to(h.dtype).reshape(h.shape) * scale


def eegnet_encoder(x, p, masks=None, drop_p=0.0, training=False, kernel_length=64, eps=1e-5, momentum=0.1):
    """oracle.cnn.eegnet_encoder (fast.py:161-167) with the two nn.Dropout as ``h * mask * scale``.  ``masks=None``:
    the oracle itself."""
    if masks is None:
        return ocnn.eegnet_encoder(x, p, training=training, eps=eps, momentum=momentum, kernel_length=kernel_length)
    scale = keep_scale(drop_p)

    def bn(h, name):
        return F.batch_norm(h, p[name + ".running_mean"], p[name + ".running_var"], p[name + ".weight"],
                            p[name + ".bias"], training, momentum, eps)
    h = x.unsqueeze(1)
    h = F.conv2d(h, p["temporal_conv.0.weight"], padding=(0, kernel_length // 2))
    h = bn(h, "temporal_conv.1")
    h = F.conv2d(h, p["spatial_conv.0.weight"], groups=p["temporal_conv.0.weight"].shape[0])
    h = F.elu(bn(h, "spatial_conv.1"))
    h = _drop(F.avg_pool2d(h, (1, 4)), masks[0], scale)
    w = p["separable_conv.0.weight"]
    h = F.conv2d(h, w, padding=(0, 8), groups=w.shape[0])
    h = F.conv2d(h, p["separable_conv.1.weight"])
    h = F.elu(bn(h, "separable_conv.2"))
    h = _drop(F.avg_pool2d(h, (1, 8)), masks[1], scale)
    h = h.mean(dim=(-2, -1))
    return F.linear(h, p["projector.2.weight"], p["projector.2.bias"])


def cvblock(x, p, masks=None, drop_p=0.0, training=False, eps=1e-5, momentum=0.1):
    """oracle.cnn.cvblock (fast.py:78-100) with the two nn.Dropout as ``h * mask * scale``.  ``masks=None``: the
    oracle itself."""
    if masks is None:
        return ocnn.cvblock(x, p, training=training, eps=eps, momentum=momentum)
    scale = keep_scale(drop_p)

    def bn(h, name):
        return F.batch_norm(h, p[name + ".running_mean"], p[name + ".running_var"], p[name + ".weight"],
                            p[name + ".bias"], training, momentum, eps)
    h = x.unsqueeze(1) if x.dim() == 3 else x
    w1 = p["conv1.weight"]
    h = bn(F.conv2d(h, w1, padding=(0, w1.shape[-1] // 2)), "bn1")
    h = F.conv2d(h, p["conv2.weight"], groups=w1.shape[0])
    h = _drop(F.avg_pool2d(F.elu(bn(h, "bn2")), (1, 8)), masks[0], scale)
    w3 = p["conv3.weight"]
    h = F.conv2d(h, w3, padding=(0, w3.shape[-1] // 2))
    h = _drop(F.avg_pool2d(F.elu(bn(h, "bn3")), (1, 2)), masks[1], scale)
    return F.linear(h.flatten(start_dim=1), p["projector.weight"], p["projector.bias"])


# ----------------------------------------------------------------------------- the GPU test's cases
class Case(NamedTuple):
    kind: str           # "eegnet" / "cvblock"
    C: int
    T: int
    K: int              # kernel_length (64 for CVBlock)
    B: int
    p: float
    F: int = 16
    stream_id: int = 41
    seed: int = 0       # torch.manual_seed of the case: initialisation, x, w, and one word of the dropout seed

    @property
    def id(self):
        return f"{self.kind}-C{self.C}-T{self.T}-K{self.K}-B{self.B}-p{self.p}"


def _eeg(C, T, K, B, p, **kw):
    return Case("eegnet", C, T, K, B, p, seed=C + T, **kw)


def _cv(C, B, **kw):
    return Case("cvblock", C, 250, 64, B, 0.5, seed=C, **kw)


# each the smallest shape that reaches a distinct code path of csrc/eegnet.hip
EEGNET_CASES = [
    _eeg(6, 250, 64, 3, 0.25),       # the FAST zone shape, bulk statistics
    _eeg(5, 65, 64, 6, 0.25),        # one-Gram statistics path (T <= 79), T3 = 2
    _eeg(7, 30, 16, 9, 0.5),         # T3 = 1, T2 = 7
    _eeg(130, 65, 64, 3, 0.25),      # wide input (C >= 128) with Gram statistics: the shape class of BASELINE config 5
    _eeg(3, 1031, 64, 2, 0.5),       # T2 = 258, T3 = 32: a second block in eeg_pool2_kernel, several 64-lane passes in pool3
    _eeg(4, 96, 32, 70, 0.25),       # B * 16 > 1024 rows: eeg_bwd3_sums_kernel's capped grid walks rows in its loop
]
CVBLOCK_CASES = [_cv(4, 3), _cv(10, 70), _cv(64, 4)]

HEAD_NAME = {"eegnet": "EEGNet_Encoder", "cvblock": "CVBlock"}
BN1_PREFIX = {"eegnet": "temporal_conv.1.", "cvblock": "bn1."}


def make_module(inn, kind, C, F, K=64, p=None):
    kw = {} if p is None else {"dropout": p}
    return inn.EEGNet_Encoder(C, F, kernel_length=K, **kw) if kind == "eegnet" else inn.CVBlock(C, F, **kw)


def randomise_bn(m, running=False):
    with torch.no_grad():
        for bn in m._bns():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.3, 0.3)
            if running:
                bn.running_mean.uniform_(-0.2, 0.2)
                bn.running_var.uniform_(0.5, 2.0)


def build_case(inn, case, running=False):
    """-> (module on the CPU with dropout on and randomised BatchNorm affine parameters, x [B, C, T], w [B, F]), the
    same on every machine: the GPU test moves them to the device, the CPU test restates them."""
    torch.manual_seed(case.seed)
    m = make_module(inn, case.kind, case.C, case.F, case.K, case.p)
    m._stream_id = case.stream_id
    randomise_bn(m, running)
    return m, torch.randn(case.B, case.C, case.T), torch.randn(case.B, case.F)


def build_head(inn, kind):
    """-> (``Head(<kind>, ocnn.ELECTRODES, ocnn.ZONES, 16)`` on the CPU: eight encoders with the class's default
    dropout, stream id 61 + zone index and randomised BatchNorm affine parameters; x [5, 64, 250]; w [5, 8, 16])."""
    torch.manual_seed(17)
    h = inn.Head(HEAD_NAME[kind], ocnn.ELECTRODES, ocnn.ZONES, 16)
    for z, e in enumerate(h.encoders.values()):
        e._stream_id = 61 + z
        randomise_bn(e)
    return h, torch.randn(5, 64, 250), torch.randn(5, 8, 16)


def build_estimator(classifier):
    """-> (``_EEGNetFeatureModel(12, 32, 5, dropout=0.25)`` on the CPU, feat [6, 12, 65], labels [6] int64)."""
    torch.manual_seed(77)
    m = classifier._EEGNetFeatureModel(12, 32, 5, dropout=0.25)
    m.net.enc._stream_id = 43
    randomise_bn(m.net.enc)
    return m, torch.randn(6, 12, 65), torch.randint(0, 5, (6,))


def run_estimator_reference(m, feat, labels, masks, drop_p):
    """EEGNet_Encoder (train mode, under ``masks``) -> Linear -> CrossEntropyLoss in fp64.  -> dict(loss, y: the
    logits, grads: {name: gradient} in the order of ``m._ordered_params()``, the order of ``m.flat_grads()``)."""
    p = ref_params(m.net.enc)
    fw, fb = (t.detach().cpu().double().requires_grad_() for t in (m.net.fc.weight, m.net.fc.bias))
    h = eegnet_encoder(feat.detach().cpu().double(), p, masks, drop_p, True, m.net.enc.kernel_length)
    logits = F.linear(h, fw, fb)
    loss = F.cross_entropy(logits, labels.cpu().long())
    loss.backward()
    names = [k for k, _ in m.net.enc.named_parameters()]
    by_param = {id(q): k for k, q in m.net.enc.named_parameters()}
    order = [by_param[id(q)] for q in m.net.enc._ordered_params()]
    assert sorted(order) == sorted(names)
    grads = {k: p[k].grad for k in order}
    grads["fc.weight"], grads["fc.bias"] = fw.grad, fb.grad
    return {"loss": loss.detach(), "y": logits.detach(), "grads": grads}


def ref_params(m):
    """The module's state as fp64 CPU leaves keyed like its state_dict; parameters ask for gradients."""
    p = {k: v.detach().cpu().clone().double() for k, v in m.state_dict().items()}
    for k, v in p.items():
        if "running" not in k and "num_batches" not in k:
            v.requires_grad_()
    return p


def reference(kind, x, p, masks, drop_p, training, K=64):
    if kind == "eegnet":
        return eegnet_encoder(x, p, masks, drop_p, training, K)
    return cvblock(x, p, masks, drop_p, training)


def grad_tol(kind, name, want, scale):
    """The bound of the p = 0 comparisons (test_eegnet_vs_oracle_shapes, test_bnheads_gpu._vs_oracle) on one parameter
    gradient: BN1's gamma / beta gradients vanish analytically (BN2 renormalises) and are held on the gradient scale."""
    floor = 5e-2 if name.startswith(BN1_PREFIX[kind]) else 1e-3
    return 1e-4 * max(float(want.abs().max()), floor * scale) + 1e-7


OUT_TOL, XGRAD_TOL, RUNNING_TOL = 1e-4, 2e-4, 1e-4


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def run_reference(kind, x, p, w, masks, drop_p, training=True, K=64, x_grad=False):
    """One reference pass: -> dict(y, grads {name: tensor}, x_grad or None); ``p`` (from ``ref_params``) keeps the
    updated running statistics.  Gradients of an earlier pass on ``p`` are dropped first."""
    for v in p.values():
        v.grad = None
    xr = x.detach().cpu().double().requires_grad_(x_grad)
    y = reference(kind, xr, p, masks, drop_p, training, K)
    (y * w.detach().cpu().double()).sum().backward()
    return {"y": y.detach(), "grads": {k: v.grad.clone() for k, v in p.items() if v.grad is not None},
            "x_grad": xr.grad}


def worst_ratio(kind, got_y, got_grads, want):
    """max over the output and every parameter gradient of error / bound (<= 1: inside the GPU test's bounds)."""
    r = {"y": rel(got_y, want["y"]) / OUT_TOL}
    scale = max(float(g.abs().max()) for g in want["grads"].values())
    for k, g in want["grads"].items():
        r[k] = float((got_grads[k].detach().cpu().double() - g).abs().max()) / grad_tol(kind, k, g, scale)
    return r
