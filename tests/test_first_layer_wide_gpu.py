"""GPU: the fp32 first-layer kernels for wide inputs -- conv5_fwd_glds_kernel (full chunks on the software-pipelined
path, a ragged last chunk on the plain loop) and conv5_wgrad_wide_kernel (zeroed dummy item, peeled last step, its own
loop for the dbias wave) -- against the fp64 oracle, through isd_featcnn_step (the first-layer output A2 is read from
the workspace) and through the layer-wise isd_conv4_forward / isd_conv4_backward of a 2-layer stack (whose output and
parameter gradients are the first layer's alone).  One zone, 32 filters, whole-row windows: the LDS-DMA kernels run.
Metric and bound are those of test_cnn_gpu.py (rel_err < 1e-4)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle import cnn as ocnn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_first_layer_golden as mk  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4
N_CLS = 5

_cases = {}


def _case(B, cin, W, big_last=False):
    """Model, inputs and the fp64 reference (A2, logits, loss, parameter gradients) of one shape; computed once."""
    key = (B, cin, W, big_last)
    if key not in _cases:
        from isd_amd.classifier import _FeatureModel
        torch.manual_seed(100 * cin + W)
        m = _FeatureModel(cin, 32, N_CLS, 4).cuda()
        gen = torch.Generator().manual_seed(B + cin + W)
        x = torch.randn(B, cin, W, generator=gen)
        if big_last:
            x[-1] *= 1e4
        y = torch.randint(0, N_CLS, (B,), generator=gen)
        p = {k: v.detach().cpu().clone().double().requires_grad_() for k, v in m.net.state_dict().items()}
        h = F.conv2d(x.double().unsqueeze(1), p["cnn.cnn1.weight"], p["cnn.cnn1.bias"])
        a2 = F.conv2d(h, p["cnn.cnn2.weight"]).squeeze(2).detach().numpy()          # [B, 32, W - 4]
        logits = ocnn.feature_cnn_logits(x.double(), p)
        loss = ocnn.cross_entropy(logits, y)
        loss.backward()
        ref = {"a2": a2, "loss": float(loss.detach()), "logits": logits.detach().numpy(),
               "grad": {"net." + k: p[k].grad.numpy() for k in p}}
        _cases[key] = (m, x.cuda().contiguous(), y.cuda(), ref)
    return _cases[key]


def _step(B, cin, W, big_last=False):
    """One isd_featcnn_step; returns (A2 [B, 32, W - 4], model, reference)."""
    import isd_amd
    import isd_amd._lib as L
    m, x, y, ref = _case(B, cin, W, big_last)
    assert L.lib().isd_featcnn_supported(m.conv_plan(x)._h, B, W, N_CLS) == 1
    hp = isd_amd.HotPath(m)
    m.flat_grads().zero_()
    out = hp.forward(x, y, want_grad=True)
    o, n = mk.a2_offset(cin), B * 32 * (W - 4)
    a2 = hp._ws["conv"][o:o + n].reshape(B, 32, W - 4).cpu().numpy()
    return a2, out, m, ref


def _check_step(B, cin, W):
    a2, out, m, ref = _step(B, cin, W)
    assert rel_err(a2, ref["a2"]) < TOL
    assert abs(float(out["loss"]) - ref["loss"]) < 1e-5
    assert rel_err(out["logits"].cpu(), ref["logits"]) < TOL
    for k, q in m.named_parameters():
        assert rel_err(q.grad.detach().cpu(), ref["grad"][k]) < TOL, k


def _check_layerwise(B, cin, W):
    """The 2-layer stack: feat = mean GELU(A2), and every parameter gradient comes from dWeff / dbeff."""
    import isd_amd.nn as inn
    p = ocnn.init_conv4_params(cin, 32, seed=cin + W, n_layers=2)
    m = inn.Conv4Layers(cin, 32, 2).cuda()
    m.load_state_dict(p)
    x = torch.randn(B, cin, W, generator=torch.Generator().manual_seed(B + 1))
    w = torch.randn(B, 32, generator=torch.Generator().manual_seed(B + 2))
    y = m(x.cuda())
    (y * w.cuda()).sum().backward()
    pr = {k: v.clone().double().requires_grad_() for k, v in p.items()}
    yr = ocnn.conv4layers(x.double(), pr, n_layers=2)
    (yr * w.double()).sum().backward()
    assert rel_err(y.detach().cpu(), yr.detach()) < TOL
    for k, q in m.named_parameters():
        assert rel_err(q.grad.cpu(), pr[k].grad) < TOL, k


def test_full_chunks():
    """cin = 64: two full 32-channel chunks (pipelined path only), one weight-gradient channel group."""
    _check_step(19, 64, 17)
    _check_layerwise(19, 64, 17)


def test_ragged_last_chunk():
    """cin = 68: two full chunks and one of 4 channels (plain loop); the second weight-gradient channel group has 4
    live channels, so three dead waves."""
    _check_step(19, 68, 17)
    _check_layerwise(19, 68, 17)


def test_forward_glds_with_generic_weight_gradient():
    """cin = 36: forward on the LDS-DMA kernel (cin > 32), weight gradient on the generic kernel (wide needs >= 64)."""
    _check_step(19, 36, 17)
    _check_layerwise(19, 36, 17)


@pytest.mark.parametrize("cin", [64, 68])
@pytest.mark.parametrize("B", [1, 9, 10, 19, 37, 2311])
def test_batches(B, cin):
    """One item; 9, 10, 19 and 37 items: up to 256 items the forward gives every item its own workgroup of four column
    tiles per wave (conv5_fwd_glds_kernel<2, 4>, mostly junk columns), and the weight gradient's workgroups get one item
    each, a stage with dead lanes in its last step.  2311 = 256 * 9 + 7: beyond 256 workgroups the forward packs nine
    13-step items into the eight tiles of conv5_fwd_glds_kernel<2, 2> (the benchmark's instance; the last workgroup has
    seven), and the weight gradient runs ragged last stages (items per workgroup not a multiple of the four per stage)."""
    _check_step(B, cin, 17)


@pytest.mark.parametrize("W", [9, 20, 7])
def test_row_lengths(W):
    """T1 = 5; T1 = 16 (no padding columns); T1 = 3 (the weight gradient's not-packed path)."""
    _check_step(10, 64, W)
    _check_layerwise(10, 64, W)


def test_ones_fragment_dbias():
    """dbeff alone (the constant-one B fragment of the dbias wave): db1 = W2^T dbeff has no other source."""
    _, _, m, ref = _step(37, 64, 17)
    k = "net.cnn.cnn1.bias"
    got = dict(m.named_parameters())[k].grad.detach().cpu()
    assert float(np.abs(ref["grad"][k]).max()) > 0
    assert rel_err(got, ref["grad"][k]) < TOL


def test_garbage_columns_do_not_leak():
    """The last trial is 1e4 times the others: junk columns past the end of a tile and the weight gradient's dummy
    item read its rows or nothing, and must not reach what is stored for the unit-scale trials."""
    a2, out, m, ref = _step(10, 64, 17, big_last=True)
    assert rel_err(a2[:-1], ref["a2"][:-1]) < TOL               # against the unit-scale trials' own magnitude
    assert rel_err(a2[-1], ref["a2"][-1]) < TOL
    assert rel_err(out["logits"][:-1].cpu(), ref["logits"][:-1]) < TOL
    for k, q in m.named_parameters():
        assert np.isfinite(q.grad.detach().cpu().numpy()).all(), k
        assert rel_err(q.grad.detach().cpu(), ref["grad"][k]) < TOL, k
