"""GPU: eval-mode forward and backward, running statistics and input gradients of the BatchNorm heads EEGNet_Encoder,
CVBlock (csrc/eegnet.hip) and HeadConv_Paper_Version (csrc/paperhead.hip) against the fp64 oracle, on the smallest shape
that reaches each kernel route (the tables of bnhead_modes_ref.py; test_bnheads_modes_cpu.py shows that each case is
well conditioned and that the running-variance cases see the N / (N - 1) factor).

Bounds (those of test_eegnet_gpu.py::test_bn_heads_input_gradient_vs_oracle and of the golden tests): output 1e-4 and
input gradient 2e-4 of the reference's largest magnitude; each parameter gradient 2e-4 of the largest gradient over all
parameters; ``running_mean`` 1e-4 of its largest magnitude; ``running_var`` 1e-4 element by element, and in the
running-variance cases 1 / 50 of what a biased variance would move the layer by where that is less.

Observed on an MI355X (worst over the cases of each head; eval / train step / running-variance cases):

===================  =========================  =========================  =========================
quantity             EEGNet_Encoder             CVBlock                    HeadConv_Paper_Version
===================  =========================  =========================  =========================
output               1.8e-7 / 2.3e-7 / 9.9e-8   7.3e-7 / 6.4e-7 / 6.9e-7   2.3e-7 / 1.0e-6 / 5.0e-7
input gradient       4.5e-7 / 6.1e-7 / -        4.3e-7 / 5.7e-7 / -        3.2e-7 / 1.4e-6 / -
parameter gradients  1.3e-7 / 2.8e-7 / -        1.8e-7 / 4.1e-7 / -        1.3e-7 / 1.9e-6 / -
running_mean         - / 1.0e-7 / 1.9e-7        - / 1.4e-7 / 8.5e-8        - / 2.4e-7 / 1.3e-7
running_var          - / 7.8e-8 / 7.4e-8        - / 7.1e-8 / 5.4e-8        - / 1.6e-7 / 1.6e-7
===================  =========================  =========================  =========================

Every test prints its own figures (``pytest -s``, lines starting with ``bnmodes``)."""
import functools

import pytest
import torch

import bnhead_modes_ref as R

pytestmark = pytest.mark.gpu

_ids = {"ids": lambda c: c.id}


@pytest.fixture(scope="module")
def inn():
    import isd_amd.nn as m
    assert torch.cuda.is_available()
    return m


@functools.lru_cache(maxsize=None)
def _case(case):
    """(module on the CPU in the case's initial state, x, w): built once, copied by every test."""
    import isd_amd.nn as inn
    return R.build_case(inn, case)


@functools.lru_cache(maxsize=None)
def _reference(case, training, momentum, eps, grads=True, biased_var=False):
    """The fp64 pass, computed once per (case, mode) and shared: nothing writes to it."""
    m, x, w = _case(case)
    return R.run_reference(case, m, x, w, training, momentum, eps, grads=grads, biased_var=biased_var)


def _module(case, momentum=None, eps=None):
    """A fresh module on the GPU in the case's initial state."""
    import isd_amd.nn as inn
    m0, x, w = _case(case)
    m = R.make_module(inn, case)
    m.load_state_dict(m0.state_dict())
    if momentum is not None:
        R.set_hyper(m, momentum, eps)
    return m.cuda(), x.cuda(), w.cuda()


def _state(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _got(m, y, x=None):
    return {"y": y.detach(), "x_grad": None if x is None else x.grad,
            "grads": {k: q.grad for k, q in m.named_parameters() if q.grad is not None},
            "buffers": {k: v for k, v in m.state_dict().items() if "running" in k}}


def _assert_within(case, tag, errs):
    worst = {}
    for name, (err, bound) in errs.items():
        q = R.quantity_class(name)
        worst[q] = max(worst.get(q, 0.0), err)
    print(f"bnmodes {case.kind} {tag}: " + ", ".join(f"{q} {e:.3e}" for q, e in worst.items()) + f"  [{case.id}]")
    bad = {k: v for k, v in errs.items() if not v[0] < v[1]}
    assert not bad, (case.id, tag, bad)


def _assert_state_unchanged(m, before):
    after = m.state_dict()
    assert set(after) == set(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k


@pytest.mark.parametrize("case", R.CASES, **_ids)
def test_eval_forward(inn, case):
    m, x, _ = _module(case)
    m.eval()
    before = _state(m)
    with torch.no_grad():
        y = m(x)
    want = _reference(case, False, *R.DEFAULT_HYPER)
    _assert_within(case, "eval forward", R.errors(_got(m, y), want, gradients=False, buffers=False))
    _assert_state_unchanged(m, before)          # running statistics and num_batches_tracked alike


@pytest.mark.parametrize("case", R.CASES, **_ids)
def test_eval_backward(inn, case):
    m, x, w = _module(case)
    m.eval()
    before = {k: v for k, v in _state(m).items() if "running" in k or "num_batches" in k}
    xg = x.clone().requires_grad_()
    y = m(xg)
    (y * w).sum().backward()
    want = _reference(case, False, *R.DEFAULT_HYPER)
    _assert_within(case, "eval backward", R.errors(_got(m, y, xg), want, buffers=False))
    # without an input gradient asked for, the parameter gradients are the same bits
    first = {k: q.grad.clone() for k, q in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    y2 = m(x)
    (y2 * w).sum().backward()
    assert torch.equal(y2.detach(), y.detach())
    for k, q in m.named_parameters():
        assert torch.equal(q.grad, first[k]), k
    after = m.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k


def _train_step(case, momentum, eps, tag):
    m, x, w = _module(case, momentum, eps)
    m.train()
    xg = x.clone().requires_grad_()
    y = m(xg)
    (y * w).sum().backward()
    want = _reference(case, True, momentum, eps)
    _assert_within(case, tag, R.errors(_got(m, y, xg), want))
    for bn in m._bns():
        assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("case", R.CASES, **_ids)
def test_train_step_with_other_momentum_and_eps(inn, case):
    _train_step(case, *R.TRAIN_HYPER, "train step")


@pytest.mark.parametrize("case", R.FIRST_OF_EACH_HEAD, **_ids)
def test_train_step_with_default_momentum_and_eps(inn, case):
    _train_step(case, *R.DEFAULT_HYPER, "train step (defaults)")


@pytest.mark.parametrize("case", R.VAR_CASES, **_ids)
def test_running_variance_is_the_unbiased_one(inn, case):
    hyper = (R.VAR_MOMENTUM, R.DEFAULT_HYPER[1])
    m, x, _ = _module(case, *hyper)
    m.train()
    with torch.no_grad():
        y = m(x)
    want = _reference(case, True, *hyper, grads=False)
    bounds = R.var_bounds(want, _reference(case, True, *hyper, grads=False, biased_var=True))
    _assert_within(case, "running variance", R.errors(_got(m, y), want, gradients=False, bounds=bounds))
    for bn in m._bns():
        assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("T", [R.CVBLOCK_T_RANGE[0] - 1, R.CVBLOCK_T_RANGE[1] + 1])
def test_cvblock_refuses_windows_outside_the_projector_range(inn, T):
    m = inn.CVBlock(4, 16, dropout=0.0).cuda()
    with pytest.raises(RuntimeError):
        m(torch.randn(2, 4, T, device="cuda"))
    assert all(int(bn.num_batches_tracked) == 0 for bn in m._bns()) and m._calls == 0


@pytest.mark.parametrize("case", R.FIRST_OF_EACH_HEAD, **_ids)
def test_disagreeing_batchnorm_hyperparameters_are_refused(inn, case):
    """A pass takes one (momentum, eps) for all its BatchNorm layers and has no cumulative average: anything else is
    refused before a counter moves, and the module works again once its layers agree."""
    m, x, w = _module(case)
    m.train()
    calls = getattr(m, "_calls", None)
    for attr, value in (("momentum", 0.3), ("eps", 1e-3), ("momentum", None)):
        saved = getattr(m._bns()[-1], attr)
        setattr(m._bns()[-1], attr, value)
        with pytest.raises(ValueError, match="BatchNorm"):
            m(x)
        setattr(m._bns()[-1], attr, saved)
        assert all(int(bn.num_batches_tracked) == 0 for bn in m._bns()) and getattr(m, "_calls", None) == calls
    y = m(x)
    want = _reference(case, True, *R.DEFAULT_HYPER)
    assert R.rel(y, want["y"]) < R.OUT_TOL
    assert all(int(bn.num_batches_tracked) == 1 for bn in m._bns())
    assert calls is None or m._calls == calls + 1
