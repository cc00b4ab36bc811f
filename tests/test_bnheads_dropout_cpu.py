"""The host reference of the BatchNorm heads' train-mode dropout (bnhead_dropout_ref.py) is right and discriminates --
no GPU: it equals oracle.cnn without masks, it equals an independent restatement on the torch sub-modules the heads
own, and for every case of test_bnheads_dropout_gpu.py a wrong mask moves the reference by at least 100x the bound
the GPU comparison is held to."""
import copy

import pytest
import torch
import torch.nn.functional as F

import bnhead_dropout_ref as R
from oracle import cnn as ocnn

MARGIN = 100.0


@pytest.fixture(scope="module")
def inn():
    import isd_amd.nn as m
    return m


def _seed(inn, stream_id, calls=1):
    """The seed of a module's ``calls``-th forward (torch.manual_seed already set by the case's builder)."""
    return inn._dropout_seed(stream_id, calls)


def _ones(kind, B, T, K):
    T2, T3 = R.geometry(kind, T, K)
    return torch.ones(B, 16, T2, dtype=torch.float64), torch.ones(B, 16, T3, dtype=torch.float64)


def test_geometry_and_streams():
    assert R.geometry("eegnet", 250, 64) == (62, 7) and R.geometry("cvblock", 250) == (31, 16)
    assert R.geometry("eegnet", 30, 16) == (7, 1) and R.geometry("eegnet", 1031, 64) == (258, 32)
    assert R.geometry("eegnet", 65, 64) == (16, 2) and R.geometry("eegnet", 96, 32) == (24, 3)
    s1, s2 = R.site_streams((1 << 63) - 1, 7)
    assert s1 == ((1 << 63) - 1 + 7 * 0xD1342543DE82EF95) % (1 << 64) and s2 == s1 ^ 0x5bd1e995
    assert R.site_streams(5, 0) == (5, 5 ^ 0x5bd1e995)
    m1, m2 = R.head_masks("eegnet", 12345, 3, 4, 250, 64, 0.25)
    assert m1.shape == (4, 16, 62) and m2.shape == (4, 16, 7) and m1.dtype == torch.float64
    assert set(m1.unique().tolist()) == {0.0, 1.0} and abs(float(m1.mean()) - 0.75) < 0.05
    # element [b, g, v] is element (b * 16 + g) * T2 + v of the stream: a longer batch extends the same sequence
    assert torch.equal(R.head_masks("eegnet", 12345, 3, 6, 250, 64, 0.25)[0][:4], m1)
    assert R.keep_scale(0.0) == 1.0 and R.keep_scale(0.5) == 2.0
    assert R.keep_scale(0.25) != 4.0 / 3.0 and abs(R.keep_scale(0.25) - 4.0 / 3.0) < 1e-7     # the fp32 quotient


@pytest.mark.parametrize("case", R.EEGNET_CASES[:3] + R.CVBLOCK_CASES[:1], ids=lambda c: c.id)
@pytest.mark.parametrize("training", [True, False])
def test_all_ones_masks_are_the_oracle_bit_for_bit(inn, case, training):
    m, x, w = R.build_case(inn, case, running=True)
    oracle = ocnn.eegnet_encoder if case.kind == "eegnet" else ocnn.cvblock
    kw = {"kernel_length": case.K} if case.kind == "eegnet" else {}
    out = []
    for fn in (lambda xx, pp: oracle(xx, pp, training=training, **kw),
               lambda xx, pp: R.reference(case.kind, xx, pp, _ones(case.kind, case.B, case.T, case.K), 0.0, training, case.K),
               lambda xx, pp: R.reference(case.kind, xx, pp, None, 0.25, training, case.K)):
        p = R.ref_params(m)
        xr = x.double().requires_grad_()
        y = fn(xr, p)
        (y * w.double()).sum().backward()
        out.append([y.detach(), xr.grad] + [p[k].grad for k in sorted(p) if p[k].grad is not None]
                   + [p[k].detach() for k in sorted(p) if "running" in k])
    for other in out[1:]:
        assert len(other) == len(out[0])
        for a, b in zip(out[0], other):
            assert torch.equal(a, b)


def _modules_eegnet(m, x, masks, scale):
    """fast.py:161-167 on the module's own torch sub-modules, the two nn.Dropout replaced by a fixed-mask multiply."""
    assert isinstance(m.spatial_conv[4], torch.nn.Dropout) and isinstance(m.separable_conv[5], torch.nn.Dropout)
    h = m.temporal_conv(x.unsqueeze(1))
    h = m.spatial_conv[:4](h) * masks[0].unsqueeze(2) * scale
    h = m.separable_conv[:5](h) * masks[1].unsqueeze(2) * scale
    return m.projector(h)


def _modules_cvblock(m, x, masks, scale):
    """fast.py:78-100 on the module's own conv / bn / projector."""
    h = m.bn1(m.conv1(x.unsqueeze(1)))
    h = F.elu(m.bn2(m.conv2(h)))
    h = F.avg_pool2d(h, (1, 8)) * masks[0].unsqueeze(2) * scale
    h = F.elu(m.bn3(m.conv3(h)))
    h = F.avg_pool2d(h, (1, 2)) * masks[1].unsqueeze(2) * scale
    return m.projector(h.flatten(start_dim=1))


@pytest.mark.parametrize("case", [R.EEGNET_CASES[0], R.EEGNET_CASES[2], R.EEGNET_CASES[5], R.CVBLOCK_CASES[0]],
                         ids=lambda c: c.id)
def test_reference_equals_the_torch_submodules_under_fixed_masks(inn, case):
    m, x, w = R.build_case(inn, case)
    masks = R.head_masks(case.kind, _seed(inn, case.stream_id), 0, case.B, case.T, case.K, case.p)
    p = R.ref_params(m)
    want = R.run_reference(case.kind, x, p, w, masks, case.p, True, case.K, x_grad=True)
    md = copy.deepcopy(m).double().train()
    xr = x.double().requires_grad_()
    y = (_modules_eegnet if case.kind == "eegnet" else _modules_cvblock)(md, xr, masks, R.keep_scale(case.p))
    (y * w.double()).sum().backward()
    assert R.rel(y, want["y"]) < 1e-10 and R.rel(xr.grad, want["x_grad"]) < 1e-10
    scale = max(float(g.abs().max()) for g in want["grads"].values())
    named = dict(md.named_parameters())
    assert set(named) == set(want["grads"])
    for k, g in want["grads"].items():
        assert float((named[k].grad - g).abs().max()) < 1e-10 * scale, k
    for k, v in md.state_dict().items():
        if "running" in k:
            assert R.rel(v, p[k]) < 1e-10, k


def _defects(kind, seed, counter, B, T, K, p):
    """{defect: (masks, drop_p)}: what a kernel that draws the wrong mask, or scales it wrongly, would compute."""
    right = R.head_masks(kind, seed, counter, B, T, K, p)
    T2, T3 = R.geometry(kind, T, K)
    s1, s2 = R.site_streams(seed, counter)
    return {
        "masks of seed + 1": (R.head_masks(kind, seed + 1, counter, B, T, K, p), p),
        "site streams exchanged": ((R.drop_keep_mask(s2, (B, 16, T2), p), R.drop_keep_mask(s1, (B, 16, T3), p)), p),
        "site-2 mask shifted by one element": ((right[0], right[1].reshape(-1).roll(1).reshape(right[1].shape)), p),
        "scale 1 in place of 1 / (1 - p)": (right, 0.0),
    }


def _assert_discriminates(kind, tag, seed, B, T, K, p, run):
    """``run(masks, drop_p)`` -> dict(y, grads) of the reference.  Every mask keeps and drops something, and every
    defect moves the output or a gradient by at least MARGIN x the GPU test's bound."""
    masks = R.head_masks(kind, seed, 0, B, T, K, p)
    for mk in masks:
        assert 0 < int(mk.sum()) < mk.numel(), tag
    want = run(masks, p)
    for name, (dm, dp) in _defects(kind, seed, 0, B, T, K, p).items():
        assert any(not torch.equal(a, b) for a, b in zip(dm, masks)) or dp != p
        got = run(dm, dp)
        ratios = R.worst_ratio(kind, got["y"], got["grads"], want)
        worst = max(ratios.values())
        print(f"{tag}: {name}: moved {worst:.3g} x bound ({max(ratios, key=ratios.get)})")
        assert worst >= MARGIN, (tag, name, ratios)


@pytest.mark.parametrize("case", R.EEGNET_CASES + R.CVBLOCK_CASES, ids=lambda c: c.id)
def test_every_gpu_case_tells_a_wrong_mask_from_the_right_one(inn, case):
    m, x, w = R.build_case(inn, case)
    for calls in (1, 2):                        # the first call of every case; the second of those that run twice
        _assert_discriminates(case.kind, f"{case.id} call {calls}", _seed(inn, case.stream_id, calls), case.B, case.T,
                              case.K, case.p,
                              lambda mk, dp: R.run_reference(case.kind, x, R.ref_params(m), w, mk, dp, True, case.K))


@pytest.mark.parametrize("counter", [1, 7])
@pytest.mark.parametrize("case", [R.EEGNET_CASES[1], R.CVBLOCK_CASES[0]], ids=lambda c: c.id)
def test_the_step_counter_moves_the_masks(inn, case, counter):
    """The device step counter enters the stream: the reference under counter 0 in place of ``counter`` misses the
    GPU test's bound by the same margin."""
    m, x, w = R.build_case(inn, case)
    seed = _seed(inn, case.stream_id)
    args = (case.B, case.T, case.K, case.p)
    want = R.run_reference(case.kind, x, R.ref_params(m), w, R.head_masks(case.kind, seed, counter, *args), case.p,
                           True, case.K)
    got = R.run_reference(case.kind, x, R.ref_params(m), w, R.head_masks(case.kind, seed, 0, *args), case.p, True,
                          case.K)
    assert max(R.worst_ratio(case.kind, got["y"], got["grads"], want).values()) >= MARGIN


@pytest.mark.parametrize("kind", ["eegnet", "cvblock"])
def test_every_zone_of_the_head_case_discriminates(inn, kind):
    h, x, w = R.build_head(inn, kind)
    for z, (area, e) in enumerate(h.encoders.items()):
        xz = x[:, h.index_dict[area]]
        _assert_discriminates(kind, f"{kind} zone {area}", _seed(inn, e._stream_id), x.shape[0], x.shape[-1], 64, e.p,
                              lambda mk, dp: R.run_reference(kind, xz, R.ref_params(e), w[:, z], mk, dp, True, 64))


def test_the_estimator_case_discriminates(inn):
    from isd_amd import classifier
    m, feat, labels = R.build_estimator(classifier)
    enc = m.net.enc
    _assert_discriminates("eegnet", "estimator", _seed(inn, enc._stream_id), 6, 65, 64, enc.p,
                          lambda mk, dp: R.run_estimator_reference(m, feat, labels, mk, dp))
