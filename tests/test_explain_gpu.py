"""GPU: expected gradients (isd_amd.explain.GradientExplainer, isd_attr_mix / isd_attr_accumulate) against the float64
restatement in test_explain_cpu.py driven by float64 autograd of the oracle, with the same draws; the kernels alone;
the estimators' ``explain``; bitwise properties; the band summary."""
import numpy as np
import pytest
import torch

from oracle import cnn as ocnn
from oracle import dsp as odsp
from test_explain_cpu import expected_gradients_reference, term_scale
from test_features_grad_cpu import band_impulse_responses, spec_s_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def isd():
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).cuda()


def gamma(S):
    return S * 2.0 ** -24 / (1.0 - S * 2.0 ** -24)


# ---------------------------------------------------------------- the kernels alone
def _kernel_problem(E, S, M, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, E)).astype(np.float32)
    bg = rng.standard_normal((M, E)).astype(np.float32)
    ridx = rng.integers(0, M, (n, S)).astype(np.int32)
    alpha = rng.random((n, S), dtype=np.float32)
    grad = rng.standard_normal((n * S, E)).astype(np.float32)
    return x, bg, ridx, alpha, grad


def _tilings(n_pairs, S):
    """Tile sizes that start and end inside trials (and one that does not divide anything)."""
    return sorted({t for t in (1, 3, S - 1, S + 1, 2 * S + 3, 64, 256) if 1 <= t < n_pairs})


KERNEL_CASES = [(E, S, M) for E in (64, 4 * 257, 795 * 3, 1, 795 * 7, 4 * 2500) for S in (1, 7, 200) for M in (1, 5)]


@pytest.mark.parametrize("E,S,M", KERNEL_CASES)
def test_mix_kernel(isd, E, S, M):
    """out = fmaf(alpha, x - b, b): within 1 ulp of float32(b + alpha (x - b)) evaluated in float64 from the fp32
    difference (a double rounding can differ from the fused result by one); rows outside the tile stay untouched."""
    from isd_amd.explain import attr_mix
    n = 3
    x, bg, ridx, alpha, _ = _kernel_problem(E, S, M, n, E + S + M)
    delta32 = (x[:, None] - bg[ridx]).astype(np.float32)                   # [n, S, E], the fp32 difference
    ref = bg[ridx].astype(np.float64) + alpha.astype(np.float64)[..., None] * delta32.astype(np.float64)
    ref = ref.reshape(n * S, E)
    xd, bd, rd, ad = dev(x), dev(bg), dev(ridx).reshape(-1), dev(alpha).reshape(-1)
    n_pairs = n * S
    for tile in [n_pairs] + _tilings(n_pairs, S):
        for p0 in sorted({0, (n_pairs - tile) // 2, n_pairs - tile}):
            out = torch.full((tile + 2, E), 7.0, device="cuda")           # a guard row on either side
            attr_mix(xd, bd, rd, ad, out[1:], p0, tile, S)
            got = out.cpu().numpy()
            assert (got[0] == 7.0).all() and (got[-1] == 7.0).all(), (tile, p0)
            want = ref[p0:p0 + tile]
            ulp = np.spacing(np.abs(want.astype(np.float32))).astype(np.float64)
            assert (np.abs(got[1:-1] - want) <= ulp).all(), (tile, p0)


@pytest.mark.parametrize("E,S,M", KERNEL_CASES)
def test_accumulate_kernel(isd, E, S, M):
    """Any tiling gives the bits of one tile, and the mean agrees with the float64 sum within the chain's bound:
    S fused multiply-adds in sequence are within gamma_S sum_s |delta_s g_s| of the exact sum (gamma_S = S u / (1 - S u),
    u = 2^-24); the fp32 difference and the final multiplication by float32(1 / S) add a few u more, covered by the
    factor 2 (S = 1 and S = 2 scale exactly)."""
    from isd_amd.explain import attr_accumulate
    n = 3
    x, bg, ridx, _, grad = _kernel_problem(E, S, M, n, 3 * E + S + M)
    xd, bd, rd, gd = dev(x), dev(bg), dev(ridx).reshape(-1), dev(grad)
    n_pairs = n * S
    one = torch.zeros((n, E), device="cuda")
    attr_accumulate(xd, bd, rd, gd, one, 0, n_pairs, S, 1.0 / S)
    for tile in _tilings(n_pairs, S):
        acc = torch.zeros((n + 2, E), device="cuda")                      # guard rows: acc[1:-1] is the target
        for p0 in range(0, n_pairs, tile):
            m = min(tile, n_pairs - p0)
            attr_accumulate(xd, bd, rd, gd[p0:p0 + m], acc[1:-1], p0, m, S, 1.0 / S)
        assert bool((acc[0] == 0).all()) and bool((acc[-1] == 0).all()), tile
        assert torch.equal(acc[1:-1], one), tile
    delta = x.astype(np.float64)[:, None] - bg.astype(np.float64)[ridx]    # [n, S, E]
    terms = delta * grad.astype(np.float64).reshape(n, S, E)
    ref, mag = terms.sum(1) / S, np.abs(terms).sum(1) / S
    bound = 2.0 * gamma(S) * mag
    err = np.abs(one.cpu().numpy() - ref)
    print(f"accumulate E={E} S={S} M={M}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    # scale = 1 keeps the sum
    keep = torch.zeros((n, E), device="cuda")
    attr_accumulate(xd, bd, rd, gd, keep, 0, n_pairs, S, 1.0)
    assert (np.abs(keep.cpu().numpy() - terms.sum(1)) <= 2.0 * gamma(S) * np.abs(terms).sum(1)).all()


# ---------------------------------------------------------------- closed forms through the explainer
class _Linear(torch.nn.Module):
    def __init__(self, W):
        super().__init__()
        self.W = torch.nn.Parameter(W)

    def forward(self, x):
        return x.flatten(1) @ self.W.flatten(1).t()


class _Quadratic(torch.nn.Module):
    def forward(self, x):
        return 0.5 * (x * x).sum((1, 2))[:, None]


def _closed_form_problem(isd, seed, n=5, Cc=3, T=795, M=4, S=24):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, Cc, T)).astype(np.float32)
    bg = rng.standard_normal((M, Cc, T)).astype(np.float32)
    ridx, alpha = isd.explain.draw_samples(n, S, M, seed)
    return rng, X, bg, ridx, alpha, S


@pytest.mark.parametrize("batch_size", [256, 37])
def test_linear_model_closed_form_and_completeness(isd, batch_size):
    rng, X, bg, ridx, alpha, S = _closed_form_problem(isd, 1)
    W = rng.standard_normal((3,) + X.shape[1:]).astype(np.float32)
    model = _Linear(torch.as_tensor(W)).cuda()
    phi = isd.explain.GradientExplainer(model, bg, batch_size=batch_size).shap_values(X, nsamples=S, rseed=1)
    assert phi.shape == X.shape + (3,) and phi.dtype == np.float32
    X64, b64, W64 = X.astype(np.float64), bg.astype(np.float64)[ridx], W.astype(np.float64)   # b64 [n, S, C, T]
    want = np.moveaxis(W64[None] * (X64 - b64.mean(1))[:, None], 1, -1)
    mag = np.moveaxis(np.abs(W64[None, None] * (X64[:, None] - b64)[:, :, None]).sum(1) / S, 1, -1)
    err = np.abs(phi - want)
    print(f"linear: max err / bound = {np.max(err / (2 * gamma(S) * mag)):.3f}")
    assert (err <= 2.0 * gamma(S) * mag).all()
    f = lambda xs: np.einsum("kct,...ct->...k", W64, xs)
    total = f(X64) - f(b64).mean(1)                                       # f_k(x) - mean_s f_k(b_r)
    # the sum over [C, T] of fp32 attributions, each within its bound
    assert (np.abs(phi.astype(np.float64).sum(axis=(1, 2)) - total) <= 2.0 * gamma(S) * mag.sum(axis=(1, 2))).all()
    ref = expected_gradients_reference(lambda xs: np.broadcast_to(W64, (len(xs),) + W64.shape), X, bg, ridx, alpha)
    assert np.abs(ref - want).max() <= 1e-12 * np.abs(want).max()


def test_quadratic_model_closed_form(isd):
    _, X, bg, ridx, alpha, S = _closed_form_problem(isd, 2)
    phi = isd.explain.GradientExplainer(_Quadratic(), bg).shap_values(X, nsamples=S, draws=(ridx, alpha))
    assert phi.shape == X.shape + (1,)
    b64 = bg.astype(np.float64)[ridx]
    delta = X.astype(np.float64)[:, None] - b64
    terms = delta * (b64 + alpha.astype(np.float64)[:, :, None, None] * delta)
    want, mag = terms.mean(1)[..., None], np.abs(terms).mean(1)[..., None]
    err = np.abs(phi - want)
    print(f"quadratic: max err / bound = {np.max(err / (2 * gamma(S) * mag)):.3f}")
    assert (err <= 2.0 * gamma(S) * mag).all()


# ---------------------------------------------------------------- real models against float64 autograd of the oracle
# Metric: per trial and class, max|phi - phi_ref| / max_s (max|delta_s| max|g_s|) of the reference.  The plain gradients
# these are averages of are held to 2e-4 of the largest gradient (test_features_grad_gpu.py, test_bnheads_gpu.py), and
# an average of S terms each within that bound is within it in this metric: 2e-4 is the ceiling.
# Measured worst values on the MI355X: FeatureCNN behind spec S 3.0e-6, FAST default / Conv4Layers
# 1.4e-7, FAST default / EEGNet_Encoder 9.0e-8, FilterbankEEGNetClassifier 1.3e-6.  The worst is more than three times
# below the ceiling, so the bound is three times the worst measured value (the arithmetic is deterministic; the
# margin is for other seeds).
REAL_MODEL_BOUND = 9e-6


def _grad64(logits_of):
    """f_grad for expected_gradients_reference from a float64 torch restatement ``logits_of(x) -> [m, K]``."""
    def f_grad(xs):
        x = torch.as_tensor(xs, dtype=torch.float64).requires_grad_(True)
        lg = logits_of(x)
        return np.stack([torch.autograd.grad(lg[:, k].sum(), x, retain_graph=True)[0].numpy()
                         for k in range(lg.shape[1])], 1)
    return f_grad


def _check_real_model(name, phi, f_grad, X, bg, ridx, alpha, bound=REAL_MODEL_BOUND):
    ref = expected_gradients_reference(f_grad, X, bg, ridx, alpha)
    scale = term_scale(f_grad, X, bg, ridx, alpha)                        # [n, K]
    assert phi.shape == ref.shape and phi.dtype == np.float32
    worst = (np.abs(phi - ref).max(axis=(1, 2)) / scale)
    print(f"{name}: worst error in the term-scale metric {worst.max():.3e} (per trial max {worst.max(1)})")
    assert np.isfinite(worst).all() and (worst <= bound).all(), worst
    return worst.max()


def _state64(m):
    return {k: v.detach().cpu().clone().double() for k, v in m.state_dict().items()}


def test_feature_cnn_behind_the_extractor(isd):
    """cfg2 cut down: 8 channels, 512 samples, 9 bands; 5 trials, 3 backgrounds, S = 16."""
    import isd_amd.nn as inn
    fs, T, Cc, bands, S = 256.0, 512, 8, odsp.BANDS_9, 16
    Xall, _ = odsp.synth_trials(8, Cc, T, fs, seed=21)
    X, bg = Xall[:5], Xall[5:]
    torch.manual_seed(5)
    net = inn.FeatureCNN(len(bands) * Cc, 32, 5).cuda().eval()
    fx = isd.FeatureExtractor(T, fs, bands)

    def model(x):
        f = fx(x)
        return net(f.view(f.shape[0], -1, f.shape[-1]))
    ridx, alpha = isd.explain.draw_samples(len(X), S, len(bg), 7)
    phi = isd.explain.GradientExplainer(model, bg).shap_values(X, nsamples=S, rseed=7)
    p, h = _state64(net), band_impulse_responses(fs, bands, T)
    f_grad = _grad64(lambda x: ocnn.feature_cnn_logits(spec_s_reference(x, fs, bands, h=h)[0], p))
    _check_real_model("FeatureCNN / spec S", phi, f_grad, X, bg, ridx, alpha)


# The BatchNorm head is the EEGNet encoder (ELU, average pooling: a smooth function of the input).  HeadConv_Paper_Version
# is not held against float64 here: its four MaxPool(1, 2) stages make the gradient piecewise, and among the ~1e6 pooling
# decisions of one explained trial some pairs tie to within fp32 rounding, where fp32 and float64 route the gradient
# to different elements.  Measured: four of five trials at 3e-8 .. 7e-8 in the metric below, one at 1.2e-3.
@pytest.mark.parametrize("head,enc", [("Conv4Layers", None), ("EEGNet_Encoder", "eegnet_encoder")])
def test_fast_default_mode(isd, head, enc):
    import isd_amd.nn as inn
    electrodes = ["Fp1", "Fp2", "F3", "F4", "C3", "C4", "O1", "O2", "Pz"]
    zones = {"Frontal": ["Fp1", "Fp2", "F3", "F4"], "Central": ["C4", "C3", "Pz"], "Occipital": ["O2", "O1"]}
    cfg = inn.fast_config(electrodes, zones, dim_cnn=16, dim_token=16, seq_len=500, n_classes=3, num_layers=1,
                          num_heads=4, dropout=0.0, head=head)
    torch.manual_seed(3)
    m = inn.FAST(cfg).cuda()
    with torch.no_grad():                                                 # eval mode reads the running statistics
        for mod in m.modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.6, 1.4)
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.3, 0.3)
    S = 16
    Xall, _ = odsp.synth_trials(8, len(electrodes), 500, 250.0, seed=22)
    X, bg = Xall[:5], Xall[5:]
    ridx, alpha = isd.explain.draw_samples(len(X), S, len(bg), 3)
    m.train()                                                             # the explainer evaluates in eval mode itself
    phi = isd.explain.GradientExplainer(m, bg).shap_values(X, nsamples=S, rseed=3)
    assert m.training
    p = _state64(m)
    names = list(zones)
    idx = [[electrodes.index(c) for c in zones[z]] for z in names]
    kw = {} if enc is None else {"encoder": getattr(ocnn, enc), "training": False}
    f_grad = _grad64(lambda x: ocnn.default_logits(x, p, names, idx, 4, 1, **kw))
    _check_real_model(f"FAST default / {head}", phi, f_grad, X, bg, ridx, alpha)


def _fit_feature_cnn(isd):
    fs, T, Cc = 256.0, 512, 8
    X, y = odsp.synth_trials(48, Cc, T, fs, seed=9)
    clf = isd.FilterbankCNNClassifier(fs=fs, max_epochs=2, batch_size=16, warmup_epochs=0, seed=1)
    return clf.fit(X, y), X


def _fit_eegnet(isd):
    fs, T, Cc = 1024.0, 2048, 3
    X, y = odsp.synth_trials(32, Cc, T, fs, seed=10)
    clf = isd.FilterbankEEGNetClassifier(bands=odsp.BANDS_40[:6], max_epochs=2, batch_size=16, warmup_epochs=0, seed=1,
                                         dropout=0.0, feature_dim=16)
    return clf.fit(X, y), X


def _fit_fast_head(isd):
    import isd_amd.nn as inn
    electrodes = ["Fp1", "Fp2", "F3", "F4", "C3", "C4", "O1", "O2", "Pz"]
    zones = {"Frontal": ["Fp1", "Fp2", "F3", "F4"], "Central": ["C4", "C3", "Pz"], "Occipital": ["O2", "O1"]}
    cfg = inn.fast_config(electrodes, zones, dim_cnn=16, dim_token=16, seq_len=500)
    X, y = odsp.synth_trials(32, len(electrodes), 500, 250.0, seed=12)
    clf = isd.FASTHeadClassifier(config=cfg, max_epochs=2, batch_size=16, warmup_epochs=0, seed=1)
    return clf.fit(X, y), X


FITS = {"feature_cnn": _fit_feature_cnn, "eegnet": _fit_eegnet, "fast_head": _fit_fast_head}


@pytest.fixture(scope="module")
def fitted(isd):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = FITS[name](isd)
        return cache[name]
    return get


def test_eegnet_feature_classifier(isd, fitted):
    clf, Xall = fitted("eegnet")
    fs, T, bands, S = 1024.0, 2048, odsp.BANDS_40[:6], 16
    X, bg = Xall[:4], Xall[4:7]
    ridx, alpha = isd.explain.draw_samples(len(X), S, len(bg), 5)
    phi = clf.explain(X, bg, nsamples=S, rseed=5)
    p, h = _state64(clf.model_.net), band_impulse_responses(fs, bands, T)

    def logits_of(x):
        feat = spec_s_reference(x, fs, bands, 1024, 960, h=h)[0]
        hid = ocnn.eegnet_encoder(feat.reshape(feat.shape[0], -1, feat.shape[-1]), p, prefix="enc.", training=False)
        return torch.nn.functional.linear(hid, p["fc.weight"], p["fc.bias"])
    _check_real_model("FilterbankEEGNetClassifier", phi, _grad64(logits_of), X, bg, ridx, alpha)


# ---------------------------------------------------------------- the estimators
def _by_hand(isd, clf, bg, **kw):
    """GradientExplainer on the same eval-mode logits, built without the estimator's help."""
    net = clf.model_.net
    if isinstance(clf, isd.FASTHeadClassifier):
        fn = lambda x: net(x, "train_head")
    else:
        def fn(x):
            f = clf._extractor(x.shape[-1])(x, fused=clf.fused)
            return net(f.view(f.shape[0], -1, f.shape[-1]))
    return isd.explain.GradientExplainer(fn, bg, **kw), net


def _snapshot(net):
    return ({k: v.clone() for k, v in net.state_dict().items()},
            [None if q.grad is None else q.grad.clone() for q in net.parameters()],
            [mod.training for mod in net.modules()],
            [{k: v for k, v in mod.__dict__.items() if k in ("_calls", "_tail_calls")} for mod in net.modules()])


def _assert_untouched(net, snap):
    sd, grads, flags, counters = snap
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    for q, g in zip(net.parameters(), grads):
        assert (q.grad is None and g is None) or torch.equal(q.grad, g)
    assert [mod.training for mod in net.modules()] == flags
    assert [{k: v for k, v in mod.__dict__.items() if k in ("_calls", "_tail_calls")} for mod in net.modules()] == counters


@pytest.mark.parametrize("name", ["feature_cnn", "eegnet", "fast_head"])
def test_estimator_explain(isd, fitted, name):
    clf, Xall = fitted(name)
    X, bg, S = Xall[:4], Xall[4:7], 8
    net = clf.model_.net
    net.train()
    snap = _snapshot(net)
    phi = clf.explain(X, bg, nsamples=S, rseed=11)
    _assert_untouched(net, snap)
    K = clf._n_classes()
    assert phi.shape == X.shape + (K,) and phi.dtype == np.float32 and np.isfinite(phi).all()
    assert np.abs(phi).max() > 0
    assert np.array_equal(clf.explain(X, bg, nsamples=S, rseed=11), phi)          # repeatable bit for bit
    assert not np.array_equal(clf.explain(X, bg, nsamples=S, rseed=12), phi)
    draws = isd.explain.draw_samples(len(X), S, len(bg), 11)
    assert np.array_equal(clf.explain(X, bg, nsamples=S, draws=draws), phi)
    ex, _ = _by_hand(isd, clf, bg)
    net.eval()
    try:
        hand = ex.shap_values(X, nsamples=S, rseed=11)
    finally:
        net.train()
    assert np.array_equal(hand, phi)
    # ranked outputs: the columns of the full result named by ranks; ranks = argsort of the logits, descending
    snap = _snapshot(net)
    top, ranks = clf.explain(X, bg, nsamples=S, ranked_outputs=2, rseed=11)
    _assert_untouched(net, snap)
    assert top.shape == X.shape + (2,) and ranks.shape == (len(X), 2) and ranks.dtype == np.int64
    dec = clf.decision_function(X)
    assert np.array_equal(ranks, np.argsort(-dec, axis=1, kind="stable")[:, :2])
    for i in range(len(X)):
        for j in range(2):
            assert np.array_equal(top[i, ..., j], phi[i, ..., ranks[i, j]]), (i, j)
    # a class column does not depend on which other classes were asked for
    only1 = isd.explain.GradientExplainer(lambda x: clf._differentiable_logits("test")[1](x)[:, 1:2], bg)
    net.eval()
    try:
        assert np.array_equal(only1.shap_values(X, nsamples=S, rseed=11)[..., 0], phi[..., 1])
    finally:
        net.train()
    # the input gradient of the same helper
    gx = clf.input_gradient(X, target=1)
    assert gx.shape == X.shape and gx.dtype == np.float32 and np.abs(gx).max() > 0


def test_fast_head_input_gradient_matches_oracle(isd, fitted):
    clf, Xall = fitted("fast_head")
    X = Xall[:4]
    cfg = clf.config
    names = list(cfg.zone_dict)
    idx = [[cfg.electrodes.index(c) for c in cfg.zone_dict[z]] for z in names]
    p = _state64(clf.model_.net)
    x = torch.as_tensor(X, dtype=torch.float64).requires_grad_(True)
    lg = ocnn.train_head_logits(x, p, names, idx, cfg.window_len, cfg.slide_step)
    ref, = torch.autograd.grad(lg[:, 2].sum(), x)
    gx = clf.input_gradient(X, target=2)
    for i in range(len(X)):
        assert np.abs(gx[i] - ref[i].numpy()).max() <= 2e-4 * np.abs(ref[i].numpy()).max(), i


def test_refusals(isd, fitted):
    clf, Xall = fitted("feature_cnn")
    X, bg = Xall[:2], Xall[2:5]
    with pytest.raises(TypeError, match="bf16"):
        isd.FilterbankCNNClassifier(precision="bf16").explain(X, bg)
    with pytest.raises(isd.NotFittedError):
        isd.FilterbankEEGNetClassifier().explain(X, bg)
    with pytest.raises(isd.NotFittedError):
        isd.FASTHeadClassifier().input_gradient(X)
    with pytest.raises(ValueError, match="like the background"):
        clf.explain(X, np.zeros((3, 8, 500), np.float32))                 # a CPU background of the wrong shape
    with pytest.raises(ValueError, match=r"\[M, C, T\]"):
        clf.explain(X, np.zeros((8, 512), np.float32))
    with pytest.raises(ValueError, match="nsamples"):
        clf.explain(X, bg, nsamples=0)
    with pytest.raises(ValueError, match="ranked_outputs"):
        clf.explain(X, bg, nsamples=2, ranked_outputs=6)
    ridx, alpha = isd.explain.draw_samples(2, 4, 3, 0)
    with pytest.raises(ValueError, match=r"lie in \[0, 3\)"):
        clf.explain(X, bg, nsamples=4, draws=(ridx + 3, alpha))
    with pytest.raises(ValueError, match="draws must be"):
        clf.explain(X, bg, nsamples=5, draws=(ridx, alpha))
    with pytest.raises(TypeError, match="differentiable"):
        isd.explain.GradientExplainer(lambda x: x.detach().sum((1,))[:, :2], bg).shap_values(X, nsamples=2)


# ---------------------------------------------------------------- bitwise properties
# Batch-invariant families: the feature classifiers.  Their extractor's input gradient is batch-invariant by test
# (test_features_grad_gpu.py::test_repeatable_and_batch_invariant) and the networks behind it compute every trial's
# row in eval mode from that row alone (Conv4Layers, the eval-mode EEGNet encoder, Linear).  FAST's transformer tail
# makes no such promise and is not declared.
@pytest.mark.parametrize("name", ["feature_cnn", "eegnet"])
def test_batch_size_does_not_change_a_bit(isd, fitted, name):
    clf, Xall = fitted(name)
    X, bg, S = Xall[:3], Xall[3:6], 24
    ref = clf.explain(X, bg, nsamples=S, rseed=4, batch_size=256)
    for bs in (7, 64):
        assert np.array_equal(clf.explain(X, bg, nsamples=S, rseed=4, batch_size=bs), ref), bs


def test_a_hip_module_graph_cannot_be_walked_twice(isd):
    """Why every class gets a forward pass of its own: the backward kernels of the HIP modules work in place on the
    workspace the forward filled and the autograd bridge releases it, so a retained graph is refused on its second walk
    (a Python error in front of any launch), while plain torch modules retain theirs."""
    import isd_amd.nn as inn
    torch.manual_seed(0)
    m = inn.Conv4Layers(6, 16).cuda().eval()
    x = torch.randn(3, 6, 250, device="cuda", requires_grad=True)
    y = m(x)
    first, = torch.autograd.grad(y[:, 0].sum(), x, retain_graph=True)
    with pytest.raises((AttributeError, RuntimeError)):
        torch.autograd.grad(y[:, 1].sum(), x, retain_graph=True)
    fresh, = torch.autograd.grad(m(x)[:, 0].sum(), x)
    assert torch.equal(first, fresh)


def test_peak_memory_stays_below_one_materialised_interpolant(isd):
    n, Cc, T, M, S = 8, 64, 512, 6, 200
    X = torch.randn(n, Cc, T, device="cuda")
    bg = torch.randn(M, Cc, T, device="cuda")
    model = _Linear(torch.randn(5, Cc, T)).cuda()
    ex = isd.explain.GradientExplainer(model, bg)
    ex.shap_values(X[:1], nsamples=2)                                     # warm the allocator's small pools
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    phi = ex.shap_values(X, nsamples=S)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"peak extra device memory {grown / 2**20:.1f} MiB vs {n * S * Cc * T * 4 / 2**20:.1f} MiB")
    assert grown < n * S * Cc * T * 4, grown
    assert phi.shape == (n, Cc, T, 5)


# ---------------------------------------------------------------- band summary
@pytest.mark.parametrize("T,sfreq", [(512, 256.0), (800, 250.0)])
def test_band_heatmap_matches_oracle(isd, T, sfreq):
    rng = np.random.default_rng(T)
    phi = rng.standard_normal((2, 5, T)).astype(np.float32)
    _, _, Z = odsp.stft(phi.astype(np.float64), sfreq, 64, 32)            # [2, 5, nfreq, J]
    ref = odsp.band_magnitude(Z, sfreq, 64, odsp.BANDS_5)                 # [2, 5, nb, J]
    got = isd.explain.band_heatmap(phi, sfreq)
    assert got.shape == ref.shape and got.dtype == np.float32
    np.testing.assert_allclose(got, ref, rtol=2e-4, atol=1e-6)
    one = isd.explain.band_heatmap(phi[0], sfreq, bands=isd.BANDS_5, nperseg=64, noverlap=32)
    assert one.shape == ref.shape[1:] and np.array_equal(one, got[0])
    assert np.array_equal(isd.explain.band_heatmap(torch.as_tensor(phi[0]).cuda(), sfreq), one)
