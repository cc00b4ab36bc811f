"""GPU: the one-call classifier step on spec-S features (isd_featcnn_step, fp32) against the fp64 oracle over the
edges of the tail kernel's item-to-wave mapping: batches that leave waves, wave pairs and whole workgroup rounds
partly empty, tile widths T1 = 1 .. 16, class counts and label types, and the inference / loss-only calls.
Metric and bounds are those of test_cnn_gpu.py::test_feature_cnn_vs_oracle."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import cnn as ocnn

pytestmark = pytest.mark.gpu

TOL = 1e-4
C = 72

_cases = {}


def _case(B, J, n_cls):
    """Model, inputs and the fp64 reference (loss, logits, parameter gradients) of one shape; computed once."""
    key = (B, J, n_cls)
    if key not in _cases:
        from isd_amd.classifier import _FeatureModel
        torch.manual_seed(1000 * J + 16 * n_cls + B % 13)
        m = _FeatureModel(C, 32, n_cls, 4).cuda()                       # .net is isd_amd.nn.FeatureCNN(72, 32, n_cls)
        gen = torch.Generator().manual_seed(B + J)
        x = torch.randn(B, C, J, generator=gen)
        y = torch.randint(0, n_cls, (B,), generator=gen)
        y[: min(B, n_cls)] = torch.arange(n_cls)[: min(B, n_cls)]       # every class that fits occurs
        p = {k: v.detach().cpu().clone().double().requires_grad_() for k, v in m.net.state_dict().items()}
        logits = ocnn.feature_cnn_logits(x.double(), p)
        loss = ocnn.cross_entropy(logits, y)
        loss.backward()
        ref = {"loss": float(loss.detach()), "logits": logits.detach().numpy(), "pred": ocnn.predict(logits.detach()).numpy(),
               "grad": {k: p[k].grad.numpy() for k, _ in m.net.named_parameters()}}
        _cases[key] = (m, x.cuda().contiguous(), y, ref)
    return _cases[key]


def _check_training_step(B, J, n_cls, label_dtype=torch.int64):
    import isd_amd
    import isd_amd._lib as L
    m, x, y, ref = _case(B, J, n_cls)
    assert L.lib().isd_featcnn_supported(m.conv_plan(x)._h, B, J, n_cls) == 1
    out = isd_amd.HotPath(m).forward(x, y.to(label_dtype).cuda(), want_grad=True)
    assert abs(float(out["loss"]) - ref["loss"]) < 1e-5
    assert rel_err(out["logits"].cpu(), ref["logits"]) < TOL
    for k, q in m.net.named_parameters():
        assert rel_err(q.grad.detach().cpu(), ref["grad"][k]) < TOL, k
    return out


@pytest.mark.parametrize("B", [1, 2, 7, 9, 17, 2059])
def test_batch_edges_vs_oracle(B):
    """A lone item (a live wave whose partner is dead), two waves of different pairs, 7 / 9 / 17 items on either side
    of one and two workgroups of eight (9 is the first batch with a live pair), and 2059 = 256 * 8 + 11: more than
    one round per workgroup, the second ragged, with waves whose partner is dead."""
    _check_training_step(B, 17, 5)


@pytest.mark.parametrize("J", [5, 9, 20])
def test_tile_widths_vs_oracle(J):
    """T1 = J - 4 = 1, 5 and 16 output steps: the extremes and the full 16-column tile."""
    _check_training_step(6, J, 5)


@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.int64])
@pytest.mark.parametrize("n_cls", [2, 5, 16])
def test_classes_and_label_types_vs_oracle(n_cls, label_dtype):
    _check_training_step(9, 17, n_cls, label_dtype)


def test_inference_call_vs_oracle():
    import isd_amd
    m, x, _, ref = _case(9, 17, 5)
    out = isd_amd.HotPath(m).forward(x)
    assert "loss" not in out
    assert rel_err(out["logits"].cpu(), ref["logits"]) < TOL
    assert np.array_equal(out["pred"].cpu().numpy(), ref["pred"])


def test_loss_only_call_vs_oracle():
    import isd_amd
    m, x, y, ref = _case(9, 17, 5)
    out = isd_amd.HotPath(m).forward(x, y.cuda())
    assert abs(float(out["loss"]) - ref["loss"]) < 1e-5
    assert rel_err(out["logits"].cpu(), ref["logits"]) < TOL
    assert np.array_equal(out["pred"].cpu().numpy(), ref["pred"])


def test_two_steps_on_the_same_inputs_are_bitwise_equal():
    import isd_amd
    m, x, y, _ = _case(2059, 17, 5)
    hp, yd = isd_amd.HotPath(m), y.cuda()
    a = hp.forward(x, yd, want_grad=True)
    ga = m.flat_grads().clone()
    b = hp.forward(x, yd, want_grad=True)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["logits"], b["logits"])
    assert torch.equal(a["pred"], b["pred"]) and torch.equal(ga, m.flat_grads())
