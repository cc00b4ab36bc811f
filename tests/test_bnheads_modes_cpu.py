"""The cases of test_bnheads_modes_gpu.py, judged on the reference alone (bnhead_modes_ref.py) -- no GPU:

* every case is well conditioned: the oracle run in fp32 stays within a quarter of each compared quantity's bound of its
  fp64 run, in every mode the GPU test uses, so a plain fp32 implementation passes with room to spare and a miss on the
  GPU is a defect of the kernels (a badly conditioned draw, a max-pool tie in the paper head for one, gets another
  ``reseed``); the paper head's max-pools moreover decide every pair the same way when their inputs are perturbed by
  a few fp32 ulps, so the verdict does not hang on one implementation's rounding;
* every running-variance case sees BatchNorm's N / (N - 1) factor: with the biased variance every layer's
  ``running_var`` misses its bound by a factor of 50;
* the window lengths CVBlock's projector takes are T = 247 .. 262;
* a head whose BatchNorm layers disagree in momentum or eps, or ask for the cumulative average (``momentum=None``),
  is refused before any counter moves."""
import pytest
import torch

import bnhead_modes_ref as R
from oracle import cnn as ocnn

CONDITION = 0.25
POOL_JITTER_DRAWS = 4


@pytest.fixture(scope="module")
def inn():
    import isd_amd.nn as m
    return m


def _assert_conditioned(case, m, x, w, tag, training, hyper, grads=True, buffers=True):
    ref64 = R.run_reference(case, m, x, w, training, *hyper, grads=grads)
    ref32 = R.run_reference(case, m, x, w, training, *hyper, dtype=torch.float32, grads=grads)
    errs = R.errors(ref32, ref64, gradients=grads, buffers=buffers)
    worst = {}
    for name, (err, bound) in errs.items():
        q = R.quantity_class(name)
        worst[q] = max(worst.get(q, 0.0), err / bound)
    print(f"{case.id} {tag}: fp32 oracle / bound: " + ", ".join(f"{q} {r:.3f}" for q, r in worst.items()))
    bad = {k: v for k, v in errs.items() if not v[0] <= CONDITION * v[1]}
    assert not bad, (case.id, tag, bad)
    if case.kind == "paper":
        # one fp32 rounding is one draw: no max-pool pair may be close enough to go the other way under another
        for seed in range(POOL_JITTER_DRAWS):
            jit = R.run_reference(case, m, x, w, training, *hyper, grads=grads, pool_jitter=seed)
            bad = {k: v for k, v in R.errors(jit, ref64, gradients=grads, buffers=buffers).items()
                   if not v[0] <= CONDITION * v[1]}
            assert not bad, (case.id, tag, "pool jitter", seed, bad)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_every_case_is_well_conditioned(inn, case):
    m, x, w = R.build_case(inn, case)
    _assert_conditioned(case, m, x, w, "eval", False, R.DEFAULT_HYPER, buffers=False)
    _assert_conditioned(case, m, x, w, "train 0.3 / 1e-3", True, R.TRAIN_HYPER)
    if case in R.FIRST_OF_EACH_HEAD:
        _assert_conditioned(case, m, x, w, "train defaults", True, R.DEFAULT_HYPER)


@pytest.mark.parametrize("case", R.CASES[:3] + R.CVBLOCK_CASES[:1] + R.PAPER_CASES[:2], ids=lambda c: c.id)
def test_eval_mode_reference_leaves_the_buffers_alone(inn, case):
    m, x, w = R.build_case(inn, case)
    ref = R.run_reference(case, m, x, w, False)
    for k, v in ref["buffers"].items():
        assert torch.equal(v, m.state_dict()[k].double()), k
    # ... and reads them: the randomised statistics are not the batch's
    train = R.run_reference(case, m, x, w, True)
    assert R.rel(train["y"], ref["y"]) > 100 * R.OUT_TOL


@pytest.mark.parametrize("case", R.VAR_CASES, ids=lambda c: c.id)
def test_running_variance_cases_see_the_unbiased_factor(inn, case):
    """With the biased variance, every BatchNorm layer of every case misses its bound (``R.var_bounds``) by
    ``R.VAR_MARGIN``, while the fp32 oracle stays within a quarter of it.  The literal ``every element moves by
    VAR_MARGIN x 1e-4`` cannot hold (a move is below 1 / (N - 1)); the layers that do reach it are printed."""
    m, x, w = R.build_case(inn, case)
    hyper = (R.VAR_MOMENTUM, R.DEFAULT_HYPER[1])
    want = R.run_reference(case, m, x, w, True, *hyper, grads=False)
    biased = R.run_reference(case, m, x, w, True, *hyper, grads=False, biased_var=True)
    ref32 = R.run_reference(case, m, x, w, True, *hyper, dtype=torch.float32, grads=False)
    assert torch.equal(biased["y"], want["y"])
    bounds = R.var_bounds(want, biased)
    assert len(bounds) == len(m._bns())
    defect = R.errors(biased, want, gradients=False, bounds=bounds)
    plain = R.errors(ref32, want, gradients=False, bounds=bounds)
    for k, (err, bound) in plain.items():
        assert err <= CONDITION * bound, (case.id, k, err, bound)
    for k, bound in bounds.items():
        v = want["buffers"][k]
        moves = (biased["buffers"][k] - v).abs() / v
        literal = float(moves.min()) >= R.VAR_MARGIN * R.RUNNING_TOL
        print(f"{case.id}: {k}: bound {bound:.3g}; the biased variance moves its elements by {float(moves.min()):.3g} .. "
              f"{float(moves.max()):.3g}{' (every element by 50 x 1e-4)' if literal else ''}; fp32 oracle "
              f"{plain[k][0]:.3g}")
        assert 0 < bound <= R.RUNNING_TOL and defect[k][0] >= R.VAR_MARGIN * bound * (1 - 1e-12), k
        assert R.rel(biased["buffers"][k.replace("_var", "_mean")], want["buffers"][k.replace("_var", "_mean")]) < 1e-12
    if case.kind == "paper":
        for seed in range(POOL_JITTER_DRAWS):
            jit = R.run_reference(case, m, x, w, True, *hyper, grads=False, pool_jitter=seed)
            for k, (err, bound) in R.errors(jit, want, gradients=False, bounds=bounds).items():
                assert err <= CONDITION * bound, (case.id, "pool jitter", seed, k)


def test_biased_variance_shim_is_the_oracle_up_to_the_factor(inn):
    """The biased restatement differs from F.batch_norm's update by exactly N / (N - 1) on the batch term."""
    case = R.EEGNET_CASES[1]
    m, x, w = R.build_case(inn, case)
    want = R.run_reference(case, m, x, w, True, 1.0, 1e-5, grads=False)       # momentum 1: the batch statistics
    biased = R.run_reference(case, m, x, w, True, 1.0, 1e-5, grads=False, biased_var=True)
    Tp = case.T + 2 * (case.K // 2) - case.K + 1
    counts = {"temporal_conv.1": case.B * case.C * Tp, "spatial_conv.1": case.B * Tp,
              "separable_conv.2": case.B * (Tp // 4 + 1)}
    for name, n in counts.items():
        k = name + ".running_var"
        assert R.rel(biased["buffers"][k] * n / (n - 1), want["buffers"][k]) < 1e-12, k


def test_cvblock_window_range(inn):
    lo, hi = R.CVBLOCK_T_RANGE
    m = inn.CVBlock(3, 16, dropout=0.0)
    p = R.ref_params(m)
    for T in (lo, 250, hi):
        assert ocnn.cvblock(torch.randn(2, 3, T, dtype=torch.float64), p).shape == (2, 16)
    for T in (lo - 1, hi + 1):
        with pytest.raises(RuntimeError):
            ocnn.cvblock(torch.randn(2, 3, T, dtype=torch.float64), p)
    assert {c.T for c in R.CVBLOCK_CASES} >= {lo, hi}


def test_case_tables_are_the_issues(inn):
    assert len(R.EEGNET_CASES) == 12 and len(R.CVBLOCK_CASES) == 3 and len(R.PAPER_CASES) == 4
    assert len({c.id for c in R.CASES + R.VAR_CASES}) == len(R.CASES) + len(R.VAR_CASES)
    for c in R.CASES + R.VAR_CASES:
        m, x, w = R.build_case(inn, c)
        assert x.shape == (c.B, c.C, c.T) and w.shape == (c.B, c.F)
        for bn in m._bns():                                      # the randomiser moved every statistic
            assert float((bn.running_var - 1).abs().min()) > 0 and float(bn.running_mean.abs().min()) > 0
            assert (bn.momentum, bn.eps) == R.DEFAULT_HYPER


# ----------------------------------------------------------------------------- refusals of _head_call
def _counters(m):
    return [int(bn.num_batches_tracked) for bn in m._bns()], getattr(m, "_calls", None)


@pytest.mark.parametrize("case", R.FIRST_OF_EACH_HEAD, ids=lambda c: c.id)
@pytest.mark.parametrize("training", [True, False])
def test_disagreeing_batchnorm_hyperparameters_are_refused(inn, case, training):
    for attr, value in (("momentum", 0.3), ("eps", 1e-3), ("momentum", None)):
        for layer in (0, -1):
            m, x, _ = R.build_case(inn, case)
            m.train(training)
            setattr(m._bns()[layer], attr, value)
            before = _counters(m)
            with pytest.raises(ValueError, match="BatchNorm"):
                m(x)
            assert _counters(m) == before
    # the cumulative average on every layer alike is refused too: the kernels have no such update
    m, x, _ = R.build_case(inn, case)
    m.train(training)
    R.set_hyper(m, None, 1e-5)
    before = _counters(m)
    with pytest.raises(ValueError, match="momentum=None"):
        m(x)
    assert _counters(m) == before
