"""GPU: the extractor's input gradient (isd_features_backward through autograd and the estimators) against float64
autograd of the spec-S restatement in test_features_grad_cpu.py, its exact properties, and its refusals."""
import numpy as np
import pytest
import torch

from oracle import cnn as ocnn
from oracle import dsp as odsp
from test_features_grad_cpu import band_impulse_responses, spec_s_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def isd():
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd


def _trials(B, Cc, T, fs, seed):
    X, _ = odsp.synth_trials(B, Cc, T, fs, seed=seed)
    return X


def _grad_gpu(isd, X, fs, bands, nperseg, noverlap, mode, precision, g, fused=None):
    fx = isd.FeatureExtractor(X.shape[-1], fs, bands, nperseg=nperseg, noverlap=noverlap, precision=precision,
                              mode=mode)
    x = torch.as_tensor(X).cuda().requires_grad_(True)
    feat = fx(x, fused=fused)
    dx, = torch.autograd.grad(feat, x, torch.as_tensor(g, dtype=torch.float32).cuda())
    return fx, feat.detach(), dx.cpu().numpy().astype(np.float64)


def _grad_ref(X, fs, bands, nperseg, noverlap, mode, g, h=None):
    x = torch.as_tensor(X, dtype=torch.float64).requires_grad_(True)
    feat, _ = spec_s_reference(x, fs, bands, nperseg, noverlap, mode=mode, h=h)
    dx, = torch.autograd.grad(feat, x, torch.as_tensor(g, dtype=torch.float64))
    return feat.detach().numpy(), dx.numpy()


def _loud(X, fs, bands, nperseg, noverlap, h=None):
    """Frames whose in-band power is within 1e4 of the median of their (band, channel) row."""
    power, _ = spec_s_reference(torch.as_tensor(X, dtype=torch.float64), fs, bands, nperseg, noverlap, mode="power",
                                h=h)
    P = power.numpy()
    return P >= np.median(P, axis=-1, keepdims=True) / 1e4


CASES = [  # T, fs, nperseg, noverlap, bands
    (512, 256.0, 64, 32, odsp.BANDS_9),                           # cfg2
    (800, 250.0, 64, 32, odsp.BANDS_5),                           # reference-native: mixed plan, Gamma's 18 bins
    (250, 250.0, 64, 32, odsp.BANDS_9),                           # ragged T
    (795, 256.0, 64, 32, odsp.BANDS_5),
    (700, 256.0, 64, 48, odsp.BANDS_9[:4]),                       # general STFT, not fusable
    (4096, 1024.0, 1024, 960, odsp.BANDS_40[:7]),                 # long rows across the fp32 / fp64 split
    (3000, 1024.0, 1024, 960, odsp.BANDS_40[:3]),                 # long and ragged
]


@pytest.mark.parametrize("mode", ["logpower", "power", "magnitude"])
@pytest.mark.parametrize("T,fs,nperseg,noverlap,bands", CASES)
@pytest.mark.parametrize("precision", ["auto", "f64"])
def test_input_gradient_matches_float64_autograd(isd, T, fs, nperseg, noverlap, bands, mode, precision):
    if precision == "f64" and (T >= 3000 and mode != "logpower"):
        pytest.skip("f64 long rows: logpower only (the float64 reference is slow at this length)")
    Cc = 3
    X = _trials(2, Cc, T, fs, seed=T + nperseg)
    h = band_impulse_responses(fs, bands, T)
    loud = _loud(X, fs, bands, nperseg, noverlap, h)
    g = np.random.default_rng(T).standard_normal(loud.shape) * loud
    fx, _, dx = _grad_gpu(isd, X, fs, bands, nperseg, noverlap, mode, precision, g)
    _, ref = _grad_ref(X, fs, bands, nperseg, noverlap, mode, g, h)
    tol = 2e-5 if fx.fb.precision == "f64" else 2e-4
    for i in range(X.shape[0]):
        err = np.abs(dx[i] - ref[i]).max() / np.abs(ref[i]).max()
        assert err <= tol, (i, err, fx.fb.precision)


def test_input_gradient_beyond_one_wave(isd):
    """135 rows: three workgroups of features_grad_kernel, the last with 7 live lanes, and a row stride of 192 (the
    cases above have at most 48 rows, one partly filled wave).  Every row against float64, each on its own scale, and
    one trial of the batch against the same trial run alone.  Measured on an MI355X (mixed plan, bound 2e-4): worst
    row 1.9e-5, worst trial 1.7e-5."""
    B, Cc, T, fs, bands, nperseg, noverlap = 5, 27, 250, 250.0, odsp.BANDS_5, 64, 32
    X = _trials(B, Cc, T, fs, seed=B * Cc + T)
    h = band_impulse_responses(fs, bands, T)
    loud = _loud(X, fs, bands, nperseg, noverlap, h)
    g = np.random.default_rng(T).standard_normal(loud.shape) * loud
    fx, _, dx = _grad_gpu(isd, X, fs, bands, nperseg, noverlap, "logpower", "auto", g)
    _, ref = _grad_ref(X, fs, bands, nperseg, noverlap, "logpower", g, h)
    tol = 2e-5 if fx.fb.precision == "f64" else 2e-4
    assert dx.shape == ref.shape == (B, Cc, T)
    err = np.abs(dx - ref).max(-1) / np.abs(ref).max(-1)                      # [B, Cc]: row by row
    print(f"beyond one wave ({fx.fb.precision}): worst row {err.max():.3e}, worst trial "
          f"{max(np.abs(dx[i] - ref[i]).max() / np.abs(ref[i]).max() for i in range(B)):.3e}")
    assert (err <= tol).all(), (np.argwhere(err > tol), err.max(), fx.fb.precision)
    _, _, alone = _grad_gpu(isd, X[3:4], fs, bands, nperseg, noverlap, "logpower", "auto", g[3:4])
    assert np.array_equal(alone[0], dx[3])


# Near-silent frames (the last frames of a short trial: P orders below the row's median) amplify the fp32 noise of P
# through 1 / (P + eps).  Unrestricted random cotangent; measured worst error over the case below: 9.2e-7 relative to
# the trial's largest gradient (MI355X), bound 5e-6.
NEAR_SILENT_TOL = 5e-6


def test_input_gradient_with_near_silent_frames(isd):
    T, fs, bands = 250, 250.0, odsp.BANDS_9
    X = _trials(2, 4, T, fs, seed=11)
    g = np.random.default_rng(5).standard_normal((2, len(bands), 4, 9))
    _, _, dx = _grad_gpu(isd, X, fs, bands, 64, 32, "logpower", "auto", g)
    _, ref = _grad_ref(X, fs, bands, 64, 32, "logpower", g)
    err = max(np.abs(dx[i] - ref[i]).max() / np.abs(ref[i]).max() for i in range(2))
    print(f"near-silent frames: max relative error {err:.3e}")
    assert err <= NEAR_SILENT_TOL


# ---------------------------------------------------------------- exact properties
def test_repeatable_and_batch_invariant(isd):
    T, fs = 800, 250.0
    fx = isd.FeatureExtractor(T, fs, odsp.BANDS_5)
    x = torch.as_tensor(_trials(8, 5, T, fs, seed=2)).cuda()
    g = torch.randn(8, 5, 5, fx.n_frames, device="cuda")
    a, b = fx.backward(x, g), fx.backward(x, g)
    assert torch.equal(a, b)
    for i in (0, 5):
        one = fx.backward(x[i:i + 1].contiguous(), g[i:i + 1].contiguous())
        assert torch.equal(one[0], a[i])


@pytest.mark.parametrize("T,nperseg,noverlap", [(512, 64, 32), (700, 64, 48), (4096, 1024, 960)])
def test_causality(isd, T, nperseg, noverlap):
    fs = 256.0 if nperseg == 64 else 1024.0
    bands = odsp.BANDS_9[:3] if nperseg == 64 else odsp.BANDS_40[2:6]
    fx = isd.FeatureExtractor(T, fs, bands, nperseg=nperseg, noverlap=noverlap)
    x = torch.as_tensor(_trials(2, 3, T, fs, seed=4)).cuda()
    hop = nperseg - noverlap
    for j in (2, fx.n_frames // 2):
        g = torch.zeros(2, fx.n_bands, 3, fx.n_frames, device="cuda")
        g[..., j] = torch.randn(2, fx.n_bands, 3, device="cuda")
        dx = fx.backward(x, g)
        end = j * hop - nperseg // 2 + nperseg - 1                  # last sample of frame j
        assert bool((dx[..., end + 1:] == 0).all())
        assert float(dx[..., :end + 1].abs().max()) > 0


@pytest.mark.parametrize("T,fs,nperseg,noverlap,bands,fused", [
    (512, 256.0, 64, 32, odsp.BANDS_9, True), (512, 256.0, 64, 32, odsp.BANDS_9, False),
    (4096, 1024.0, 1024, 960, odsp.BANDS_40[:7], True), (700, 256.0, 64, 48, odsp.BANDS_9, None)])
def test_forward_with_grad_is_bitwise_the_no_grad_forward(isd, T, fs, nperseg, noverlap, bands, fused):
    fx = isd.FeatureExtractor(T, fs, bands, nperseg=nperseg, noverlap=noverlap)
    x = torch.as_tensor(_trials(3, 4, T, fs, seed=6)).cuda()
    plain = fx(x, fused=fused)
    xg = x.clone().requires_grad_(True)
    withg = fx(xg, fused=fused)
    assert withg.grad_fn is not None and torch.equal(withg.detach(), plain)
    via = isd.extract_features(xg, fs=fs, bands=bands, nperseg=nperseg, noverlap=noverlap, fused=fused)
    assert via.grad_fn is not None and torch.equal(via.detach(), plain)


def test_full_cfg2_batch_needs_no_filtered_signal_tensor(isd):
    B, Cc, T = 4096, 64, 512
    fx = isd.FeatureExtractor(T, 256.0, odsp.BANDS_9)
    x = torch.randn(B, Cc, T, device="cuda", requires_grad=True)
    feat = fx(x)
    g = torch.randn_like(feat)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    dx, = torch.autograd.grad(feat, x, g)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    assert grown < B * fx.n_bands * Cc * T * 4, grown
    assert bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0


# ---------------------------------------------------------------- refusals
def test_refusals(isd):
    fx = isd.FeatureExtractor(512, 256.0, odsp.BANDS_9)
    x = torch.randn(2, 8, 512, device="cuda", requires_grad=True)
    with pytest.raises(TypeError):
        fx(x, out_dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        fx(x, out=torch.empty(2, 9, 8, fx.n_frames, device="cuda"))
    with torch.no_grad():                                          # no gradient asked for: the old behaviour
        assert fx(x, out_dtype=torch.bfloat16).dtype == torch.bfloat16
    with pytest.raises(isd.NotFittedError):
        isd.FilterbankCNNClassifier().input_gradient(np.zeros((1, 8, 512), np.float32))
    with pytest.raises(TypeError):
        isd.FilterbankCNNClassifier(precision="bf16").input_gradient(np.zeros((1, 8, 512), np.float32))


# ---------------------------------------------------------------- end to end through the estimators
def _net_state(clf):
    return {k: v.detach().cpu().double() for k, v in clf.model_.net.state_dict().items()}


def _check_estimator(clf, X, fs, bands, nperseg, noverlap, logits_of, tol):
    params = list(clf.model_.net.parameters())
    grads_before = [None if p.grad is None else p.grad.clone() for p in params]
    bufs_before = {k: v.clone() for k, v in clf.model_.net.state_dict().items()}
    flags_before = [m.training for m in clf.model_.net.modules()]
    dec = clf.decision_function(X)
    pred = dec.argmax(1)
    gx = clf.input_gradient(X)
    assert gx.shape == X.shape and gx.dtype == np.float32
    p = _net_state(clf)
    x = torch.as_tensor(X, dtype=torch.float64).requires_grad_(True)
    feat, _ = spec_s_reference(x, fs, bands, nperseg, noverlap)
    logits = logits_of(feat, p)
    assert np.abs(logits.detach().numpy() - dec).max() <= 1e-3 * max(1.0, np.abs(dec).max())
    ref, = torch.autograd.grad(logits.gather(1, torch.as_tensor(pred)[:, None]).sum(), x, retain_graph=True)
    ref = ref.numpy()
    for i in range(len(X)):
        assert np.abs(gx[i] - ref[i]).max() <= tol * np.abs(ref[i]).max(), i
    # a fixed target: class 1 for every trial
    g1 = clf.input_gradient(X, target=1)
    ref1, = torch.autograd.grad(logits[:, 1].sum(), x)
    assert np.abs(g1 - ref1.numpy()).max() <= tol * np.abs(ref1.numpy()).max()
    # the HIP logits on the differentiated path are decision_function's
    fx = clf._extractor(X.shape[-1])
    with torch.no_grad():
        f = fx(torch.as_tensor(X).cuda())
        clf.model_.net.eval()
        lg = clf.model_.net(f.view(f.shape[0], -1, f.shape[-1])).cpu().numpy()
        for m, w in zip(clf.model_.net.modules(), flags_before):
            m.training = w
    assert np.abs(lg - dec).max() <= 1e-5 * max(1.0, np.abs(dec).max())
    for p_, g_ in zip(params, grads_before):
        assert (p_.grad is None and g_ is None) or torch.equal(p_.grad, g_)
    for k, v in clf.model_.net.state_dict().items():
        assert torch.equal(v, bufs_before[k]), k
    assert [m.training for m in clf.model_.net.modules()] == flags_before


def test_feature_cnn_classifier_input_gradient(isd):
    fs, T, Cc = 256.0, 512, 8
    X, y = odsp.synth_trials(48, Cc, T, fs, seed=9)
    clf = isd.FilterbankCNNClassifier(fs=fs, max_epochs=2, batch_size=16, warmup_epochs=0, seed=1)
    clf.fit(X, y)
    _check_estimator(clf, X[:6], fs, odsp.BANDS_9, 64, None,
                     lambda feat, p: ocnn.feature_cnn_logits(feat, p), 2e-3)


def test_eegnet_classifier_input_gradient(isd):
    fs, T, Cc = 1024.0, 2048, 3
    bands = odsp.BANDS_40[:6]
    X, y = odsp.synth_trials(32, Cc, T, fs, seed=10)
    clf = isd.FilterbankEEGNetClassifier(bands=bands, max_epochs=2, batch_size=16, warmup_epochs=0, seed=1,
                                         dropout=0.0, feature_dim=16)

    def logits_of(feat, p):
        h = ocnn.eegnet_encoder(feat.reshape(feat.shape[0], -1, feat.shape[-1]), p, prefix="enc.", training=False)
        return torch.nn.functional.linear(h, p["fc.weight"], p["fc.bias"])

    clf.fit(X, y)
    _check_estimator(clf, X[:4], fs, bands, 1024, 960, logits_of, 2e-3)
