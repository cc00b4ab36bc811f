"""TSception without a GPU: the module's surface against the torch restatement (tests/tsception_ref.py), the
estimator's sklearn protocol, and the library's envelope checks."""
import ctypes as C

import numpy as np
import pytest
import torch

from tsception_ref import TSception as RefTSception

SHAPES = [(64, 800, 250, 15, 15, 32, 26402), (4, 96, 64, 3, 3, 8, 362), (7, 250, 250, 15, 15, 32, 7052)]
ORDER = (["%s.0.%s" % (b, w) for b in ("Tception1", "Tception2", "Tception3", "Sception1", "Sception2", "fusion_layer")
          for w in ("weight", "bias")]
         + ["%s.%s" % (b, w) for b in ("BN_t", "BN_s", "BN_fusion") for w in ("weight", "bias")]
         + ["fc.0.weight", "fc.0.bias", "fc.3.weight", "fc.3.bias"])


def test_exports_exist():
    import isd_amd
    assert isd_amd.nn.TSception is not None and isd_amd.TSceptionClassifier is not None
    assert issubclass(isd_amd.TSceptionPath, isd_amd.HotPath)


@pytest.mark.parametrize("Cn,T,fs,nT,nS,hid,count", SHAPES)
def test_state_dict_matches_the_restatement_and_loads_both_ways(monkeypatch, Cn, T, fs, nT, nS, hid, count):
    import isd_amd
    from isd_amd import _lib

    def no_library():
        raise AssertionError("constructing / loading a TSception on the CPU must not touch the library")
    monkeypatch.setattr(_lib, "lib", no_library)
    torch.manual_seed(1)
    ref = RefTSception(5, (1, Cn, T), fs, nT, nS, hid, 0.5)
    m = isd_amd.nn.TSception(5, (1, Cn, T), fs, nT, nS, hid, 0.5)
    a, b = ref.state_dict(), m.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
    assert sum(p.numel() for p in m.parameters()) == count
    assert [k for k, _ in m.named_parameters()] == ORDER
    m.load_state_dict(a, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, a[k]), k
    ref2 = RefTSception(5, (1, Cn, T), fs, nT, nS, hid, 0.5)
    ref2.load_state_dict(m.state_dict(), strict=True)
    flat = m.flat_params()
    assert flat.numel() == count and not flat.is_cuda
    assert torch.equal(flat, torch.cat([a[k].reshape(-1) for k in ORDER]))
    assert torch.equal(m.flat_buffers(), torch.cat([a[f"{bn}.{r}"] for bn in ("BN_t", "BN_s", "BN_fusion")
                                                    for r in ("running_mean", "running_var")]))


def test_shapes_outside_the_model_or_the_envelope_are_refused():
    import isd_amd
    T = isd_amd.nn.TSception
    with pytest.raises(ValueError, match="two rows"):
        T(5, (1, 3, 800), 250, 15, 15, 32, 0.5)
    with pytest.raises(ValueError, match="valid"):
        T(5, (1, 8, 131), 250, 15, 15, 32, 0.5)              # 131 - 125 + 1 = 7 < 8 valid samples
    with pytest.raises(ValueError, match="fusion"):
        T(5, (1, 8, 11), 8, 3, 3, 8, 0.5)                    # taps 4 / 2 / 1: pooled 1 + 1 + 1 = 3 -> 1 -> 0
    with pytest.raises(NotImplementedError, match="num_T"):
        T(5, (1, 8, 800), 250, 17, 15, 32, 0.5)
    with pytest.raises(NotImplementedError, match="hidden"):
        T(5, (1, 8, 800), 250, 15, 15, 65, 0.5)
    with pytest.raises(NotImplementedError, match="channels"):
        T(5, (1, 129, 800), 250, 15, 15, 32, 0.5)
    T(5, (1, 2, 800), 250, 1, 1, 1, 0.5)


def test_estimator_follows_the_sklearn_protocol():
    import isd_amd
    base = pytest.importorskip("sklearn.base")
    clf = isd_amd.TSceptionClassifier(max_epochs=3, batch_size=20, num_T=6, hidden=16, dropout_rate=0.0)
    p = clf.get_params()
    assert p["sampling_rate"] == 250.0 and p["num_T"] == 6 and p["num_S"] == 15 and p["hidden"] == 16
    assert p["dropout_rate"] == 0.0 and p["n_classes"] == 5 and p["max_epochs"] == 3 and p["batch_size"] == 20
    twin = base.clone(clf)
    assert twin is not clf and twin.get_params() == p and twin.model_ is None
    assert clf.set_params(num_S=7, lr=1e-3) is clf and clf.num_S == 7 and clf.lr == 1e-3
    with pytest.raises(ValueError, match="invalid parameter"):
        clf.set_params(nonsense=1)
    X = np.zeros((4, 8, 128), np.float32)
    with pytest.raises(isd_amd.NotFittedError):
        clf.predict(X)
    with pytest.raises(isd_amd.NotFittedError):
        clf.decision_function(X)
    with pytest.raises(NotImplementedError):
        clf.input_gradient(X)
    with pytest.raises(NotImplementedError):
        clf.explain(X, X)


def test_every_entry_point_is_declared_and_the_envelope_is_checked_without_a_gpu():
    from isd_amd import _lib
    names = ["isd_tsception_" + n for n in ("plan_create", "plan_destroy", "param_count", "buffer_count",
                                            "workspace_bytes", "forward", "backward")]
    for n in names:
        assert n in _lib.SIGNATURES, n
    L = _lib.lib()
    h = C.c_void_p()
    good = dict(C=64, T=800, k1=125, k2=62, k3=31, nT=15, nS=15, hid=32, ncls=5)
    assert L.isd_tsception_plan_create(C.byref(h), *good.values()) == 0
    assert L.isd_tsception_param_count(h) == 26402 and L.isd_tsception_buffer_count(h) == 90
    assert L.isd_tsception_workspace_bytes(h, 4) > 0
    assert L.isd_tsception_plan_destroy(h) == 0
    for bad in (dict(C=3), dict(C=1), dict(C=129), dict(k1=513), dict(k3=0), dict(T=131), dict(T=140, k1=125), dict(nT=17),
                dict(nS=0), dict(hid=65), dict(ncls=17)):
        args = dict(good, **bad)
        if bad == dict(T=140, k1=125):
            args.update(k2=125, k3=125)                      # 16 valid samples per bank: 2 + 2 + 2 pooled -> 3 -> 0
        h = C.c_void_p()
        rc = L.isd_tsception_plan_create(C.byref(h), *args.values())
        assert rc < 0 and not h.value, bad
        assert len(L.isd_last_error()) > 0, bad


def _real_operands(L, h, B, Cn, T, ncls):
    """Operands of a pass as real, correctly sized buffers -- on the GPU where there is one -- so that a refusal that
    ever stopped coming before the launch would meet valid memory.  Returns (tensors kept alive, pointers)."""
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    ws_floats = int(L.isd_tsception_workspace_bytes(h, min(B, 350))) // 4 * (1 + B // 350)
    ts = [torch.zeros(B, Cn, T, device=dev), torch.zeros(int(L.isd_tsception_param_count(h)), device=dev),
          torch.ones(int(L.isd_tsception_buffer_count(h)), device=dev), torch.zeros(B, ncls, device=dev),
          torch.zeros(ws_floats, device=dev)]
    return ts, [t.data_ptr() for t in ts]


def test_a_zone_batch_refuses_the_model():
    """The zone-batched launches record the per-zone heads only: a TSception call inside a batch fails loudly."""
    from isd_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    assert L.isd_tsception_plan_create(C.byref(h), 8, 128, 32, 16, 8, 6, 7, 16, 5) == 0
    keep, (x, params, bufs, out, ws) = _real_operands(L, h, 4, 8, 128, 5)
    assert L.isd_zone_batch_begin() == 0
    try:
        rc = L.isd_tsception_forward(h, x, params, bufs, out, ws, 4, 0, 0.1, 1e-5, 0.0, 0, None)
        assert rc == _lib.ISD_ERR_UNSUPPORTED and b"zone batch" in L.isd_last_error()
        rc = L.isd_tsception_temporal_probe(h, x, params, ws, 4, 0, None)
        assert rc == _lib.ISD_ERR_UNSUPPORTED and b"zone batch" in L.isd_last_error()
    finally:
        L.isd_zone_batch_abort()
        L.isd_tsception_plan_destroy(h)
    del keep


def test_more_than_350_trials_per_pass_are_refused_by_the_library():
    """350 trials, the notebook's full batch, is the largest batch the kernels have run at: the bound is enforced."""
    import isd_amd
    from isd_amd import _lib
    assert isd_amd.nn.TSception.MAX_BATCH == isd_amd.TSceptionPath.MAX_BATCH == 350
    L = _lib.lib()
    h = C.c_void_p()
    assert L.isd_tsception_plan_create(C.byref(h), 4, 96, 32, 16, 8, 3, 3, 8, 5) == 0
    try:
        assert L.isd_tsception_workspace_bytes(h, 350) > 0
        assert L.isd_tsception_workspace_bytes(h, 351) < 0 and b"350" in L.isd_last_error()
        keep, (x, params, bufs, out, ws) = _real_operands(L, h, 351, 4, 96, 5)
        for rc in (L.isd_tsception_forward(h, x, params, bufs, out, ws, 351, 0, 0.1, 1e-5, 0.0, 0, None),
                   L.isd_tsception_backward(h, x, params, out, params, ws, 351, 0.0, 0, None),
                   L.isd_tsception_temporal_probe(h, x, params, ws, 351, 0, None)):
            assert rc == _lib.ISD_ERR_INVALID and b"350" in L.isd_last_error()
        del keep
    finally:
        L.isd_tsception_plan_destroy(h)
