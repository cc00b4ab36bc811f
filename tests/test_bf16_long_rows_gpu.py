"""GPU: bf16 feature maps for the long-row extractor and the EEGNet / CVBlock head that reads them (BASELINE config 5).

Both rules are exact, so every comparison here is bit for bit:
  * map:  the long-row bf16 map is the fp32 map rounded to nearest even (fused_long_kernel / fused_rows4_kernel with
    out16, both band sets of a mixed-precision plan);
  * head: the bf16-input kernels widen each value to fp32 on load and then compute what the fp32 kernels compute, so
    a bf16 input xb gives the bits of the fp32 head on xb.float() -- output, running statistics, num_batches_tracked
    and every parameter gradient.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import dsp as odsp

pytestmark = pytest.mark.gpu

FS, T5, C5, NPERSEG, NOVERLAP = 1024.0, 4096, 128, 1024, 960


@pytest.fixture(scope="module")
def isd():
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd


def _maps(fx, x):
    """(fp32 map, bf16 map, launched family of the bf16 call)."""
    from isd_amd import _lib
    f32 = fx(x, fused=True)
    f16 = fx(x, fused=True, out_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    return f32, f16, int(_lib.lib().isd_features_fused_last_path())


def _check_map(fx, x):
    f32, f16, path = _maps(fx, x)
    assert path == 3                                       # the long-row block-sum kernels wrote the bf16 map
    assert f16.dtype == torch.bfloat16 and f16.shape == f32.shape
    assert bool(torch.isfinite(f32).all())
    assert torch.equal(f16, f32.to(torch.bfloat16))        # torch's conversion is round-to-nearest-even
    out = torch.empty_like(f16)
    assert fx(x, fused=True, out=out) is out and torch.equal(out, f16)
    return f32, f16


# ----------------------------------------------------------------------------------------------------- map
def test_cfg5_rows_bf16_map_is_the_rounded_fp32_map(isd):
    """Config-5 rows (128 ch x 4096 samples, 40 bands, 1024/960): the AUTO rule puts some bands in fp64, so both band
    sets (the float and the double instances of fused_rows4_kernel) write through the band map."""
    X, _ = odsp.synth_trials(3, C5, T5, FS, seed=11)
    fx = isd.FeatureExtractor(T5, FS, isd.BANDS_40, nperseg=NPERSEG, noverlap=NOVERLAP)
    assert fx.fb.precision == "mixed"
    _check_map(fx, torch.from_numpy(X).cuda())


@pytest.mark.parametrize("T,fs,nperseg,noverlap,bands", [
    (4096, 1024.0, 1024, 960, odsp.BANDS_40[:7]),       # stress shape; bands on both sides of the fp32 / fp64 split
    (4096, 1024.0, 1024, 960, odsp.BANDS_40[20:24]),    # fp32 bands only
    (3000, 1024.0, 1024, 960, odsp.BANDS_40[:3]),       # ragged row: fused_long_kernel, last pass and block partial
    (1500, 512.0, 256, 192, [("a", 6.0, 10.0), ("b", 20.0, 24.0)]),   # one pass, 4 blocks per frame
    (1536, 1024.0, 1024, 960, odsp.BANDS_40[:5]),       # whole 512-sample passes: fused_rows4_kernel
    (2048, 512.0, 256, 192, [("a", 6.0, 10.0), ("b", 20.0, 24.0), ("c", 30.0, 38.0)]),
])
def test_long_rows_bf16_map_shapes(isd, T, fs, nperseg, noverlap, bands):
    """The shapes of the fp32 long-row test: 3 trials x 5 channels leave a ragged last quad of rows."""
    X, _ = odsp.synth_trials(3, 5, T, fs, seed=T)
    fx = isd.FeatureExtractor(T, fs, bands, nperseg=nperseg, noverlap=noverlap)
    assert fx.can_fuse
    _check_map(fx, torch.from_numpy(X).cuda())


def test_long_rows_bf16_map_unaligned_input(isd):
    """x one float off a 16-byte boundary: the scalar-load instance (fused_long_kernel<..., false>)."""
    X, _ = odsp.synth_trials(2, 6, T5, FS, seed=5)
    buf = torch.empty(X.size + 1, device="cuda")
    x = buf[1:].view(X.shape)
    x.copy_(torch.from_numpy(X))
    assert x.data_ptr() % 16 != 0
    fx = isd.FeatureExtractor(T5, FS, odsp.BANDS_40[:7], nperseg=NPERSEG, noverlap=NOVERLAP)
    f32, f16 = _check_map(fx, x)
    assert torch.equal(f16, fx(x.contiguous().clone(), out_dtype=torch.bfloat16))   # the aligned kernels agree


@pytest.mark.parametrize("mode", ["power", "magnitude"])
@pytest.mark.parametrize("T", [4096, 3000])
def test_long_rows_bf16_map_other_modes(isd, mode, T):
    X, _ = odsp.synth_trials(3, 5, T, FS, seed=7)
    fx = isd.FeatureExtractor(T, FS, odsp.BANDS_40[:7], nperseg=NPERSEG, noverlap=NOVERLAP, mode=mode)
    _check_map(fx, torch.from_numpy(X).cuda())


@pytest.mark.slow
def test_cfg5_full_batch_bf16_map(isd):
    """B = 2048 at config 5: every value of the bf16 map against the rounded fp32 map."""
    gen = torch.Generator(device="cuda").manual_seed(2048)
    x = torch.randn(2048, C5, T5, device="cuda", generator=gen)
    fx = isd.FeatureExtractor(T5, FS, isd.BANDS_40, nperseg=NPERSEG, noverlap=NOVERLAP)
    f32, f16, path = _maps(fx, x)
    assert path == 3
    assert torch.equal(f16, f32.to(torch.bfloat16))


# ----------------------------------------------------------------------------------------------------- head
def _randomise_bn(m):
    with torch.no_grad():
        for bn in m._bns():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.3, 0.3)
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 2.0)


def _twins(make, seed):
    torch.manual_seed(seed)
    a = make().cuda()
    _randomise_bn(a)
    b = make().cuda()
    b.load_state_dict(a.state_dict())
    return a, b


def _feature_like(B, C, T, seed):
    """A bf16 tensor with the spread of log band power features."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(B, C, T, device="cuda", generator=gen) * 3.0 - 12.0).to(torch.bfloat16)


def _train_pass(m, x, w):
    m.train()
    for p in m.parameters():
        p.grad = None
    y = m(x)
    (y * w).sum().backward()
    return (y.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()},
            {k: v.clone() for k, v in m.named_buffers()})


def _assert_same_pass(pa, pb):
    ya, ga, ba = pa
    yb, gb, bb = pb
    assert torch.equal(ya, yb)
    assert ga.keys() == gb.keys() and ba.keys() == bb.keys()
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    for k in ba:                                           # running statistics and num_batches_tracked
        assert torch.equal(ba[k], bb[k]), k


def _check_twins(a, b, xb, w):
    assert xb.dtype == torch.bfloat16
    pa, pb = _train_pass(a, xb, w), _train_pass(b, xb.float(), w)
    _assert_same_pass(pa, pb)
    assert int(a._bns()[0].num_batches_tracked) == 1
    a.eval()
    b.eval()
    with torch.no_grad():
        assert torch.equal(a(xb), b(xb.float()))


# The EEGNet pooling stages need T >= 27, so the one-Gram-matrix statistics kernel is reached with 2..5 tiles
# (T = 30, 50, 65); T = 200 takes the bulk + edge statistics; C < 128 the per-tile spatial product, C >= 128 the
# whole-row one (eeg_spatial_rows_kernel<5>, the config-5 shape 5120 x 65).
@pytest.mark.parametrize("C,T,K,B", [(24, 30, 64, 6), (24, 50, 32, 5), (24, 65, 64, 7), (9, 200, 64, 5),
                                     (64, 65, 64, 4), (64, 333, 32, 3), (5120, 65, 64, 8), (200, 81, 16, 3)])
def test_eegnet_bf16_input_gives_the_bits_of_the_fp32_head(isd, C, T, K, B):
    import isd_amd.nn as inn
    a, b = _twins(lambda: inn.EEGNet_Encoder(C, 16, kernel_length=K, dropout=0.0), C + T)
    xb = _feature_like(B, C, T, C * T)
    w = torch.randn(B, 16, device="cuda")
    _check_twins(a, b, xb, w)


def test_cvblock_bf16_input_gives_the_bits_of_the_fp32_head(isd):
    import isd_amd.nn as inn
    a, b = _twins(lambda: inn.CVBlock(12, 16, dropout=0.0), 250)
    xb = _feature_like(4, 12, 250, 250)
    w = torch.randn(4, 16, device="cuda")
    _check_twins(a, b, xb, w)


def test_eegnet_bf16_input_with_dropout(isd):
    """Dropout masks are keyed by the module's stream id and call counter: the same module, its state and counter put
    back between the two passes."""
    import isd_amd.nn as inn
    torch.manual_seed(3)
    m = inn.EEGNet_Encoder(40, 16, dropout=0.25).cuda()
    _randomise_bn(m)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    calls = m._calls
    xb = _feature_like(6, 40, 65, 1)
    w = torch.randn(6, 16, device="cuda")
    pa = _train_pass(m, xb, w)
    m.load_state_dict(sd)
    m._calls = calls
    pb = _train_pass(m, xb.float(), w)
    _assert_same_pass(pa, pb)
    m.load_state_dict(sd)
    m._calls = calls
    p0 = _train_pass(m, xb.float(), torch.zeros_like(w))
    assert not torch.equal(p0[0], _train_pass(m, xb.float(), w)[0])    # the masks do change from call to call


# ------------------------------------------------------------------------------------------------ refusals
def test_bf16_head_refusals(isd):
    import isd_amd.nn as inn
    m = inn.EEGNet_Encoder(8, 16, dropout=0.0).cuda()
    xb = _feature_like(3, 8, 65, 0)
    calls = m._calls
    m.train()
    with pytest.raises(TypeError, match="cannot require grad"):
        m(xb.clone().requires_grad_())
    m.eval()
    with pytest.raises(TypeError, match="eval-mode parameter gradients"):
        m(xb)
    for dt in (torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32 or bfloat16"):
            m(xb.to(dt))
    assert m._calls == calls and int(m._bns()[0].num_batches_tracked) == 0   # nothing ran
    with torch.no_grad():
        assert m(xb).shape == (3, 16)                      # eval without gradients is taken
    m.train()
    for p in m.parameters():
        p.requires_grad_(False)
    assert m(xb).shape == (3, 16)                          # train mode without any gradient, too


def test_backward_x_refuses_a_bf16_plan(isd):
    from isd_amd import _lib
    from isd_amd.nn import EEGNetPlan
    B, Cc, T = 2, 8, 65
    plan = EEGNetPlan(Cc, 16, 64, T, dtype=torch.bfloat16)
    L = _lib.lib()
    x = _feature_like(B, Cc, T, 0)
    flat = torch.zeros(plan.n_params, device="cuda")
    dflat = torch.zeros_like(flat)
    dout = torch.zeros(B, 16, device="cuda")
    dx = torch.zeros(B, Cc, T, device="cuda")
    ws = torch.zeros(int(L.isd_eegnet_workspace_bytes(plan._h, B)) // 4, device="cuda")
    rc = L.isd_eegnet_backward_x(plan._h, x.data_ptr(), flat.data_ptr(), dout.data_ptr(), dflat.data_ptr(),
                                 dx.data_ptr(), ws.data_ptr(), B, 1, 0.0, 0, None)
    assert rc == _lib.ISD_ERR_UNSUPPORTED
    with pytest.raises(_lib.IsdUnsupported, match="bf16"):
        _lib.check(rc)
    with pytest.raises(_lib.IsdError):
        _lib.check(L.isd_eegnet_plan_set_input_dtype(plan._h, 7))


# ----------------------------------------------------------------------------------------------- estimator
def test_eegnet_path_step_on_a_bf16_map(isd):
    """One training step of EEGNet_Encoder -> Linear -> CE on the extractor's bf16 map against the fp32 path fed
    map.float(): the same loss and the same flat parameters after AdamW, bit for bit."""
    from isd_amd.classifier import _EEGNetFeatureModel
    X, y = odsp.synth_trials(16, C5, T5, FS, seed=4)
    fx = isd.FeatureExtractor(T5, FS, isd.BANDS_40, nperseg=NPERSEG, noverlap=NOVERLAP)
    f16 = fx(torch.from_numpy(X).cuda(), out_dtype=torch.bfloat16).view(16, 40 * C5, 65)
    yt = torch.from_numpy(np.asarray(y)).cuda().long()
    models = []
    for _ in range(2):
        torch.manual_seed(0)
        models.append(_EEGNetFeatureModel(40 * C5, 32, 5, dropout=0.0).cuda())
    m16, m32 = models
    assert torch.equal(m16.flat_params(), m32.flat_params())
    t16, t32 = isd.Trainer(m16), isd.Trainer(m32)
    l16 = float(t16.step(f16, yt)["loss"])
    l32 = float(t32.step(f16.float(), yt)["loss"])
    assert l16 == l32 and np.isfinite(l16)
    assert torch.equal(m16.flat_params(), m32.flat_params())
    assert torch.equal(m16.net.enc.flat_buffers(), m32.net.enc.flat_buffers())
    e16, e32 = t16.path.forward(f16), t32.path.forward(f16.float())                  # eval mode
    assert torch.equal(e16["logits"], e32["logits"]) and torch.equal(e16["pred"], e32["pred"])


def test_filterbank_eegnet_classifier_bf16(isd):
    """fit / predict of the config-5 estimator with precision='bf16' on the reduced synthetic task of the fp32 test."""
    X, y = odsp.synth_trials(48, C5, T5, FS, seed=2)
    clf = isd.FilterbankEEGNetClassifier(max_epochs=60, batch_size=48, warmup_epochs=2, seed=3, dropout=0.0, lr=5e-3,
                                         precision="bf16")
    assert clf.fit(X, y) is clf
    assert clf.history_[-1] < 1.3                                                     # from ln 5 = 1.61
    first_loss = clf.history_[-1]
    first_params = clf.model_.flat_params().clone()
    clf.fit(X, y)
    assert len(clf.history_) == 1 and clf.history_[-1] == first_loss
    assert torch.equal(clf.model_.flat_params(), first_params)
    pred = clf.predict(X)
    assert pred.shape == (48,) and pred.dtype == np.int64 and (pred == y).mean() > 0.4
    assert clf.score(X, y) == float((pred == y).mean())
    feats, per_batch = clf._prepare_fit(torch.from_numpy(X).cuda())                   # the training-set cache
    assert feats.dtype == torch.bfloat16 and feats.shape == (48, 40 * C5, 65)
    assert clf.extract_features(torch.from_numpy(X[:2]).cuda()).dtype == torch.bfloat16
