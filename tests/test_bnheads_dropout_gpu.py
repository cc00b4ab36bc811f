"""GPU parity of EEGNet_Encoder and CVBlock (csrc/eegnet.hip) in train mode WITH dropout against fp64 torch under the
same masks.  The masks are counter-based: seven kernels (eeg_pool2 / eeg_pool3 / cv_pool3 forward; eeg_bwd3_sums /
eeg_bwd_sep / eeg_bwd_pool2 / cv_dy3 backward) each evaluate drop_scale(stream, element index, p) on an index they
form their own way, so forward and backward are right only if all agree element for element.  bnhead_dropout_ref.py
recomputes the masks on the host and restates the networks; test_bnheads_dropout_cpu.py shows that each case here
misses its bound by >= 100x under a wrong seed, exchanged site streams, a site-2 mask shifted by one element, or a
missing 1 / (1 - p).  Bounds: those of the p = 0 comparisons (test_eegnet_gpu.py, test_bnheads_gpu.py)."""
import pytest
import torch

import bnhead_dropout_ref as R
from oracle import cnn as ocnn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inn():
    import isd_amd.nn as m
    assert torch.cuda.is_available()
    return m


def _call_masks(inn, m, kind, B, T, counter=0):
    """The masks of the forward ``m`` has just run (the call counter moves before it is used), each keeping and
    dropping at least one element."""
    seed = inn._dropout_seed(m._stream_id, m._calls)
    masks = R.head_masks(kind, seed, counter, B, T, getattr(m, "kernel_length", 64), m.p)
    for mk in masks:
        assert 0 < int(mk.sum()) < mk.numel()
    return masks


def _check(tag, kind, y, grads, want, x_grad=None, bufs=None, ref_bufs=None):
    """Output, every parameter gradient (and the input gradient, the running statistics) inside the bounds; prints
    the worst error / bound of the case first."""
    ratios = R.worst_ratio(kind, y, grads, want)
    if x_grad is not None:
        ratios["x.grad"] = R.rel(x_grad, want["x_grad"]) / R.XGRAD_TOL
    for k, v in (bufs or {}).items():
        if "running" in k:
            ratios[k] = R.rel(v, ref_bufs[k]) / R.RUNNING_TOL
        if "num_batches_tracked" in k:
            assert int(v) == int(ref_bufs[k]), k
    worst = max(ratios, key=ratios.get)
    print(f"{tag}: output {ratios['y'] * R.OUT_TOL:.2e} (bound {R.OUT_TOL:.0e}); worst error / bound "
          f"{ratios[worst]:.3f} ({worst})")
    bad = {k: round(v, 3) for k, v in ratios.items() if not v < 1.0}
    assert not bad, (tag, bad)


def _grads(m):
    return {k: q.grad for k, q in m.named_parameters()}


def _train_pass(inn, m, kind, x, w, p, K, counter=0, x_grad=False, tag=""):
    """One train-mode forward + backward of ``m`` on the GPU against the reference under the host masks of that call.
    ``p``: the reference's parameter dict (its running statistics follow the module's from pass to pass)."""
    m.zero_grad(set_to_none=True)
    xg = x.cuda().requires_grad_(x_grad and x.dtype == torch.float32)
    y = m(xg)
    (y * w.cuda()).sum().backward()
    masks = _call_masks(inn, m, kind, x.shape[0], x.shape[-1], counter)
    for k in p:
        if "num_batches_tracked" in k:
            p[k] += 1
    want = R.run_reference(kind, x, p, w, masks, m.p, True, K, x_grad=x_grad)
    _check(tag, kind, y, _grads(m), want, xg.grad if x_grad else None, m.state_dict(), p)


@pytest.mark.parametrize("case", R.EEGNET_CASES + R.CVBLOCK_CASES, ids=lambda c: c.id)
def test_train_mode_dropout_vs_fp64_under_host_masks(inn, case):
    m, x, w = R.build_case(inn, case)
    m = m.cuda().train()
    assert m.p == case.p > 0
    _train_pass(inn, m, case.kind, x, w, R.ref_params(m), case.K, tag=case.id)
    assert m._calls == 1 and m._stream_id == case.stream_id      # the masks test_bnheads_dropout_cpu.py discriminates on


@pytest.mark.parametrize("case", [R.EEGNET_CASES[0], R.CVBLOCK_CASES[0]], ids=lambda c: c.id)
def test_input_gradient_under_dropout_then_parameter_only_backward(inn, case):
    """isd_eegnet_backward_x in train mode with dropout on, then the parameter-only backward on the next call: the
    call counter has advanced, so that call draws other masks."""
    m, x, w = R.build_case(inn, case)
    m = m.cuda().train()
    p = R.ref_params(m)
    _train_pass(inn, m, case.kind, x, w, p, case.K, x_grad=True, tag=case.id + " with x.grad")
    first = inn._dropout_seed(m._stream_id, m._calls)
    _train_pass(inn, m, case.kind, x, w, p, case.K, tag=case.id + " next call, parameters only")
    assert m._calls == 2 and inn._dropout_seed(m._stream_id, m._calls) != first


@pytest.mark.parametrize("case", [R.EEGNET_CASES[0]._replace(p=0.5), R.EEGNET_CASES[1], R.CVBLOCK_CASES[0],
                                  R.CVBLOCK_CASES[0]._replace(p=0.25)], ids=lambda c: c.id)
def test_eval_mode_ignores_p(inn, case):
    """Modules built with dropout 0.25 / 0.5 on non-trivial running statistics, in eval(): the forward without
    gradients, and the forward that keeps its activations plus the input-gradient backward, are the oracle's."""
    m, x, w = R.build_case(inn, case, running=True)
    m = m.cuda().eval()
    assert m.p == case.p > 0
    p = R.ref_params(m)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    want = R.run_reference(case.kind, x, p, w, None, m.p, False, case.K, x_grad=True)
    with torch.no_grad():
        y = m(x.cuda())
    assert R.rel(y, want["y"]) < R.OUT_TOL
    xg = x.cuda().requires_grad_()
    y = m(xg)
    (y * w.cuda()).sum().backward()
    _check(case.id + " eval", case.kind, y, _grads(m), want, xg.grad)
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k                       # eval mode moves no statistics


@pytest.mark.parametrize("when", ["before the first forward", "after the first forward"])
@pytest.mark.parametrize("case", [R.EEGNET_CASES[1], R.CVBLOCK_CASES[0]], ids=lambda c: c.id)
def test_device_step_counter_enters_the_masks(inn, case, when):
    """``set_seed_counter(t)``: the int64 device word is read by every pass (eager here; a captured graph bumps it
    between replays) -- a plan made after the call and a plan cached before it both receive it, and None takes it
    away again."""
    m, x, w = R.build_case(inn, case)
    m = m.cuda().train()
    p = R.ref_params(m)
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    if when == "after the first forward":
        _train_pass(inn, m, case.kind, x, w, p, case.K, tag=f"{case.id} no counter yet")
        assert len(m._plans) == 1
    m.set_seed_counter(t)
    for v in (0, 1, 7):
        t.fill_(v)
        _train_pass(inn, m, case.kind, x, w, p, case.K, counter=v, tag=f"{case.id} counter {v} set {when}")
    assert len(m._plans) == 1
    m.set_seed_counter(None)                                      # t still holds 7: nobody reads it any more
    _train_pass(inn, m, case.kind, x, w, p, case.K, counter=0, tag=f"{case.id} counter cleared")


def test_bf16_input_map_under_dropout(inn):
    """A bfloat16 input is widened on load, exactly: train mode, parameter gradients only, against the reference on
    ``x.bfloat16().double()`` at the fp32 bounds."""
    case = R.EEGNET_CASES[1]
    m, x, w = R.build_case(inn, case)
    m = m.cuda().train()
    xb = x.bfloat16()
    assert not torch.equal(xb.float(), x)
    _train_pass(inn, m, case.kind, xb, w, R.ref_params(m), case.K, tag=case.id + " bf16 x")
    assert (case.T, torch.bfloat16) in m._plans


@pytest.mark.parametrize("kind", ["eegnet", "cvblock"])
def test_zone_batched_head_under_dropout(inn, kind, monkeypatch):
    """Head(<kind>, 64 electrodes, 8 zones, 16) on the default, zone-batched route (launch i of all zones is one
    kernel): zone z's features and its encoder's gradients against the reference on that zone's channels under the
    masks of that encoder's own (stream id, call counter)."""
    monkeypatch.delenv("ISD_ZONE_BATCH_OFF", raising=False)
    h, x, w = R.build_head(inn, kind)
    h = h.cuda().train()
    encs = list(h.encoders.values())
    refs = [R.ref_params(e) for e in encs]
    xc = x.cuda()
    assert h._zone_batchable(encs, xc)
    f = h(xc)
    (f * w.cuda()).sum().backward()
    assert f.shape == (5, 8, 16)
    for z, (area, e) in enumerate(h.encoders.items()):
        assert e._calls == 1 and e._stream_id == 61 + z
        masks = _call_masks(inn, e, kind, 5, 250)
        for k in refs[z]:
            if "num_batches_tracked" in k:
                refs[z][k] += 1
        want = R.run_reference(kind, x[:, h.index_dict[area].cpu()], refs[z], w[:, z], masks, e.p, True, 64)
        _check(f"{kind} zone {area}", kind, f[:, z], _grads(e), want, None, e.state_dict(), refs[z])


def test_estimator_step_under_dropout(inn):
    """The estimator's own step (classifier.EEGNetPath: encoder -> Linear -> softmax-CE, no autograd) with dropout on:
    loss, logits and the flat gradient block against the fp64 restatement under the host masks."""
    from isd_amd import classifier
    m, feat, labels = R.build_estimator(classifier)
    m = m.cuda()
    enc = m.net.enc
    out = m.make_path().forward(feat.cuda(), labels.cuda(), want_grad=True)
    assert enc._calls == 1 and enc.p == 0.25
    masks = _call_masks(inn, enc, "eegnet", 6, 65)
    want = R.run_estimator_reference(m, feat, labels, masks, enc.p)
    flat, got, off = m.flat_grads(), {}, 0
    for k, g in want["grads"].items():
        got[k] = flat[off:off + g.numel()].view(g.shape)
        off += g.numel()
    assert off == flat.numel()
    print(f"estimator: loss error {abs(float(out['loss']) - float(want['loss'])):.2e} (bound 1e-5)")
    assert abs(float(out["loss"]) - float(want["loss"])) < 1e-5
    assert torch.equal(out["pred"].cpu(), want["y"].argmax(1))
    _check("estimator step", "eegnet", out["logits"], got, want)
