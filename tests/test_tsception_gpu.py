"""TSception on the GPU against the torch restatement (tests/tsception_ref.py) evaluated on the CPU in fp64.

Tolerance rule: a quantity passes within max(1e-4, 4 x the fp32 restatement's own deviation from fp64); 1e-4 is the
project's fp32 gate, the factor 4 covers a second fp32 summation order (a wrong term shows at 1e-2 or more), and a case
whose fp32 deviation exceeds 1.25e-4 fails as badly conditioned (``tsception_ref.bound``).  Outputs are compared with
``rel_err``, parameter gradients as  max |d| / max(max |want|, 1e-3 x the largest gradient magnitude)."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err
from tsception_ref import FixedMask, as_double, bound, class_tone_trials, grad_errors, make_ref, train_pass

pytestmark = pytest.mark.gpu

CASES = [(3, 4, 96, 64, 3, 3, 8),            # every pool drops a remainder
         (2, 7, 250, 250, 15, 15, 32),       # odd C: Sception2 drops a channel; taps 125 / 62 / 31
         (5, 6, 200, 100, 4, 5, 8),          # num_T != num_S; taps 50 / 25 / 12
         (70, 10, 160, 64, 15, 15, 32),      # more trials than one workgroup's share
         (2, 2, 600, 1024, 2, 2, 4),         # taps 512 / 256 / 128; C = 2
         (6, 128, 160, 64, 16, 16, 8),       # widest spatial contraction; 16 filters
         (4, 64, 800, 250, 15, 15, 32)]      # the reference's trial


@functools.lru_cache(maxsize=None)
def _train_reference(case):
    """(fp32 restatement, x, w, fp64 pass, fp32 pass) of one case, computed once and never modified."""
    B, C, T, fs, nT, nS, hid = case
    ref = make_ref(C, T, fs, nT, nS, hid, seed=B + C)
    g = torch.Generator().manual_seed(T)
    x = torch.randn(B, C, T, generator=g)
    w = torch.randn(B, 5, generator=g)
    return ref, x, w, train_pass(as_double(ref), x, w), train_pass(ref, x, w)


def _gpu_model(ref, dropout=0.0):
    import isd_amd
    C = ref.Sception1[0].weight.shape[2]
    nT, nS = ref.BN_t.num_features, ref.BN_s.num_features
    hid, ncls = ref.fc[0].out_features, ref.fc[3].out_features
    k1 = ref.Tception1[0].weight.shape[3]
    m = isd_amd.nn.TSception(ncls, (1, C, 8 * k1), 2 * k1, nT, nS, hid, dropout)
    assert m.taps == tuple(b[0].weight.shape[3] for b in (ref.Tception1, ref.Tception2, ref.Tception3))
    m.load_state_dict(ref.state_dict(), strict=True)
    return m.cuda()


def _gpu_train_pass(m, x, w):
    m.train()
    m.zero_grad(set_to_none=True)
    logits = m(x.cuda())
    (logits * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().double() for k, p in m.named_parameters()}
    bufs = {k: v.detach().cpu().clone() for k, v in m.named_buffers()}
    return logits.detach().cpu().double(), grads, bufs


def _check_pass(got, want, own, tag):
    """``got`` (GPU), ``want`` (fp64) and ``own`` (the fp32 restatement) are (logits, grads, buffers)."""
    dev = rel_err(own[0], want[0])
    err = rel_err(got[0], want[0])
    print(f"{tag}: logits err {err:.2e} (fp32 restatement {dev:.2e})")
    assert err < bound(dev), f"{tag}: logits {err:.2e}"
    ge, gd = grad_errors(got[1], want[1]), grad_errors(own[1], want[1])
    print(f"{tag}: worst gradient err {max(ge.values()):.2e} (fp32 restatement {max(gd.values()):.2e})")
    for k in ge:
        assert ge[k] < bound(gd[k]), f"{tag}: d{k} {ge[k]:.2e} (fp32 restatement {gd[k]:.2e})"
    for k, v in want[2].items():
        if k.endswith("num_batches_tracked"):
            assert int(got[2][k]) == int(v), k
        else:
            e = rel_err(got[2][k], v)
            assert e < bound(rel_err(own[2][k], v)), f"{tag}: {k} {e:.2e}"


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_train_forward_gradients_and_running_statistics_vs_fp64(case):
    ref, x, w, want, own = _train_reference(case)
    got = _gpu_train_pass(_gpu_model(ref), x, w)
    _check_pass(got, want, own, str(case))


@pytest.mark.parametrize("case", [CASES[0], CASES[6]], ids=lambda c: "x".join(map(str, c)))
def test_eval_forward_vs_fp64(case):
    B, C, T, fs, nT, nS, hid = case
    ref, x, _, _, _ = _train_reference(case)
    ref = as_double(ref).float()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for bn in (ref.BN_t, ref.BN_s, ref.BN_fusion):
            bn.running_mean.copy_(torch.randn(bn.num_features, generator=g) * 0.2)
            bn.running_var.copy_(torch.rand(bn.num_features, generator=g) * 1.5 + 0.5)
    m = _gpu_model(ref).eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        got = m(x.cuda())
        got4 = m(x.cuda()[:, None])
        want = as_double(ref).eval()(x.double()[:, None])
        own = ref.eval()(x[:, None])
    assert torch.equal(got, got4)
    err, dev = rel_err(got.cpu(), want), rel_err(own, want)
    print(f"{case}: eval logits err {err:.2e} (fp32 restatement {dev:.2e})")
    assert err < bound(dev)
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k                   # eval mode updates nothing


def test_eval_logits_do_not_depend_on_the_batch():
    ref, x, _, _, _ = _train_reference(CASES[3])
    m = _gpu_model(ref).eval()
    xg = x.cuda()
    with torch.no_grad():
        whole = m(xg)
        halves = torch.cat([m(xg[:35].contiguous()), m(xg[35:].contiguous())])
    assert rel_err(halves.cpu(), whole.cpu()) < 1e-5


def test_a_training_step_is_bitwise_repeatable():
    ref, x, w, _, _ = _train_reference(CASES[3])
    a = _gpu_train_pass(_gpu_model(ref), x, w)
    b = _gpu_train_pass(_gpu_model(ref), x, w)
    assert torch.equal(a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_dropout_mask_recovered_from_the_output():
    B, C, T, fs, p = 32, 4, 96, 64, 0.5
    ref = make_ref(C, T, fs, 3, 3, 8, n_classes=8, seed=11)
    with torch.no_grad():
        ref.fc[3].weight.copy_(torch.eye(8))
        ref.fc[3].bias.zero_()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, C, T, generator=g)
    w = torch.randn(B, 8, generator=g)
    m = _gpu_model(ref, dropout=p).train()
    m.p = 0.0
    with torch.no_grad():
        plain = m(x.cuda()).cpu()                               # logits = the hidden units themselves
    m.load_state_dict(ref.state_dict())                         # (the running statistics moved)
    m.p = p
    logits = m(x.cuda())
    (logits * w.cuda()).sum().backward()
    got = (logits.detach().cpu().double(), {k: q.grad.cpu().double() for k, q in m.named_parameters()})
    positive = plain > 0
    keep = torch.where(positive, logits.detach().cpu() != 0, torch.ones_like(positive))
    share = float(keep[positive].float().mean())
    print(f"kept {share:.3f} of {int(positive.sum())} positive units")
    assert 0.35 <= share <= 0.65
    passes = []
    for r in (as_double(ref), ref):
        r = as_double(r).to(next(r.parameters()).dtype)
        r.fc[2] = FixedMask(keep, p)
        passes.append(train_pass(r, x, w))
    want, own = passes
    err, dev = rel_err(got[0], want[0]), rel_err(own[0], want[0])
    print(f"dropout: logits err {err:.2e} (fp32 restatement {dev:.2e})")
    assert err < bound(dev)
    ge, gd = grad_errors(got[1], want[1]), grad_errors(own[1], want[1])
    print(f"dropout: worst gradient err {max(ge.values()):.2e} (fp32 restatement {max(gd.values()):.2e})")
    for k in ge:
        assert ge[k] < bound(gd[k]), f"d{k} {ge[k]:.2e}"
    with torch.no_grad():
        again = m(x.cuda()).cpu()
        assert not torch.equal(again != 0, logits.detach().cpu() != 0)          # a second call draws another mask
        m.eval()
        e1 = m(x.cuda())
        m.p = 0.0
        assert torch.equal(e1, m(x.cuda()))                     # eval() ignores p


@functools.lru_cache(maxsize=None)
def _tone_task():
    X, y = class_tone_trials(40, 8, 128, 64.0, seed=0)
    Xf, _ = class_tone_trials(64, 8, 128, 64.0, seed=1)
    return torch.from_numpy(X), torch.from_numpy(y), torch.from_numpy(Xf)


def _adamw_losses(r, X, y, steps):
    opt = torch.optim.AdamW(r.parameters(), lr=5e-4, weight_decay=1e-2)
    dt = next(r.parameters()).dtype
    out = []
    r.train()
    for _ in range(steps):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(r(X.to(dt)[:, None]), y)
        loss.backward()
        opt.step()
        out.append(float(loss.detach()))
    return np.array(out)


def _eval_check(m_logits, state, X, make, tag):
    r32 = make()
    r32.load_state_dict(state)
    with torch.no_grad():
        want = as_double(r32).eval()(X.double()[:, None])
        own = r32.eval()(X[:, None])
    err, dev = rel_err(m_logits, want), rel_err(own, want)
    print(f"{tag}: eval logits err {err:.2e} (fp32 restatement {dev:.2e})")
    assert err < bound(dev)
    return want


def test_trainer_three_steps_match_adamw_on_the_restatement():
    import isd_amd
    X, y, Xf = _tone_task()
    make = lambda: make_ref(8, 128, 64, 6, 7, 16, seed=21)                      # noqa: E731
    m = _gpu_model(make())
    tr = isd_amd.Trainer(m, lr=5e-4, weight_decay=1e-2)
    xg, yg = X.cuda(), y.cuda()
    got = np.array([float(tr.step(xg, yg)["loss"]) for _ in range(3)])
    want = _adamw_losses(as_double(make()), X, y, 3)
    own = _adamw_losses(make(), X, y, 3)
    err, dev = rel_err(got, want), rel_err(own, want)
    print(f"trainer: losses {got} err {err:.2e} (fp32 restatement {dev:.2e})")
    assert err < bound(dev)
    assert int(m.BN_t.num_batches_tracked) == 3
    m.eval()
    with torch.no_grad():
        logits = m(Xf.cuda()).cpu()
    state = {k: v.cpu() for k, v in m.state_dict().items()}
    _eval_check(logits, state, Xf, make, "trainer")


def test_estimator_fit_predict_decision_function():
    import isd_amd
    X, y, Xf = _tone_task()
    clf = isd_amd.TSceptionClassifier(max_epochs=3, batch_size=20, dropout_rate=0.0, sampling_rate=64.0, num_T=6,
                                      num_S=7, hidden=16, warmup_epochs=1)
    assert clf.fit(X.numpy(), y.numpy()) is clf
    assert len(clf.history_) == 1 and np.isfinite(clf.history_).all()
    first = {k: v.cpu().clone() for k, v in clf.model_.state_dict().items()}
    dec = clf.decision_function(Xf.numpy())
    assert dec.shape == (64, 5) and dec.dtype == np.float32
    make = lambda: make_ref(8, 128, 64, 6, 7, 16)                               # noqa: E731
    want = _eval_check(dec, first, Xf, make, "estimator").numpy()
    top = np.sort(want, axis=1)
    sure = (top[:, -1] - top[:, -2]) >= 1e-3
    assert sure.mean() >= 0.9
    pred = clf.predict(Xf.numpy())
    assert pred.dtype == np.int64 and (pred[sure] == want.argmax(1)[sure]).all()
    assert 0.0 <= clf.score(Xf.numpy(), np.zeros(64, np.int64)) <= 1.0
    clf.fit(X.numpy(), y.numpy())                                               # a second fit starts from scratch
    for k, v in clf.model_.state_dict().items():
        assert torch.equal(v.cpu(), first[k]), k


def test_the_batch_bound_itself_is_checked_and_one_more_trial_is_refused():
    """350 trials per pass is the bound the library enforces: the step is checked AT it, and 351 trials raise."""
    import isd_amd
    case = (350, 4, 96, 64, 3, 3, 8)
    assert case[0] == isd_amd.nn.TSception.MAX_BATCH
    ref, x, w, want, own = _train_reference(case)
    m = _gpu_model(ref)
    _check_pass(_gpu_train_pass(m, x, w), want, own, str(case))
    tracked = int(m.BN_t.num_batches_tracked)
    x351 = torch.zeros(351, 4, 96, device="cuda")
    with pytest.raises(ValueError, match="at most 350"):
        m(x351)
    with pytest.raises(ValueError, match="at most 350"):
        m.make_path().forward(x351)
    assert int(m.BN_t.num_batches_tracked) == tracked
    clf = isd_amd.TSceptionClassifier(max_epochs=1, batch_size=351, sampling_rate=64.0, num_T=3, num_S=3, hidden=8)
    with pytest.raises(ValueError, match="at most 350"):
        clf.fit(x351, torch.zeros(351, dtype=torch.int64))


def test_refusals():
    import isd_amd
    ref, x, _, _, _ = _train_reference(CASES[0])
    m = _gpu_model(ref)
    xg = x.cuda()
    with pytest.raises(NotImplementedError, match="input gradient"):
        m(xg.clone().requires_grad_())
    with pytest.raises(TypeError, match="float32"):
        m(xg.bfloat16())
    with pytest.raises(TypeError, match="CUDA"):
        m(x)
    with pytest.raises(ValueError, match="channels"):
        m(xg[:, :3].contiguous())
    path = m.make_path()
    assert isinstance(path, isd_amd.TSceptionPath)
    with pytest.raises(TypeError, match="bfloat16"):
        path.forward(xg.bfloat16())
    with pytest.raises(ValueError, match="contiguous"):
        path.forward(xg.transpose(0, 1).contiguous().transpose(0, 1))
    with pytest.raises(NotImplementedError, match="graph"):
        m.set_seed_counter(torch.zeros(1, dtype=torch.int64, device="cuda"))
    tracked = int(m.BN_t.num_batches_tracked)
    out = path.forward(xg)                                                      # no labels: eval mode
    assert set(out) == {"logits", "pred"} and int(m.BN_t.num_batches_tracked) == tracked
    out = path.forward(xg, torch.zeros(3, dtype=torch.int64, device="cuda"), want_grad=True)
    assert set(out) == {"logits", "pred", "loss"} and int(m.BN_t.num_batches_tracked) == tracked + 1
