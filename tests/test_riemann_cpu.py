"""isd_amd.riemann on the host: argument handling of the estimators and functions, the declared ABI, and self-checks
of the NumPy restatement (tests/riemann_ref.py) that the GPU tests compare against.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import isd_amd
import riemann_ref as ref
from isd_amd import _lib
from isd_amd import riemann as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spd_stack(n, C, seed):
    return ref.covariances(ref.synthetic_trials(n, C, 4 * C + 3, seed))


# ------------------------------------------------------------------------------------------------ the declared ABI
def test_header_and_binding_declare_the_entry_points():
    header = open(os.path.join(ROOT, "include", "isd_hip.h")).read()
    for name, nargs in (("isd_spd_congruence", 9), ("isd_spd_eigfun", 9)):
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert m, f"{name} is not declared in isd_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    for k, name in enumerate(("ISD_SPD_LOG", "ISD_SPD_SQRT", "ISD_SPD_INVSQRT", "ISD_SPD_INV", "ISD_SPD_NONE")):
        assert re.search(name + r" = %d\b" % k, header)
    for k, name in enumerate(("ISD_SPD_FULL", "ISD_SPD_TANGENT", "ISD_SPD_NOOUT")):
        assert re.search(name + r" = %d\b" % k, header)
    assert (rm.SPD_LOG, rm.SPD_SQRT, rm.SPD_INVSQRT, rm.SPD_INV, rm.SPD_NONE) == (0, 1, 2, 3, 4)
    assert (rm.SPD_FULL, rm.SPD_TANGENT, rm.SPD_NOOUT) == (0, 1, 2)
    assert "#define ISD_ABI_VERSION 1" in header


def test_exported_with_pyriemann_signatures():
    assert isd_amd.riemann is rm and "riemann" in isd_amd.__all__

    def sig(f):
        return [(k, p.default) for k, p in list(inspect.signature(f).parameters.items())[1:]]
    assert sig(rm.Covariances.__init__) == [("estimator", "scm")]
    assert sig(rm.TangentSpace.__init__) == [("metric", "riemann"), ("tsupdate", False)]
    assert sig(rm.MDM.__init__) == [("metric", "riemann")]
    assert [k for k, _ in sig(rm.MDM.fit)] == ["X", "y", "sample_weight"]
    p = inspect.signature(rm.mean_riemann).parameters
    assert list(p)[:6] == ["covs", "tol", "maxiter", "init", "sample_weight", "groups"]
    assert (p["tol"].default, p["maxiter"].default) == (1e-8, 50)


# ------------------------------------------------------------------------------------------- sklearn protocol
@pytest.mark.parametrize("est", [rm.Covariances(), rm.TangentSpace(), rm.MDM()])
def test_get_set_params_and_clone(est):
    base = pytest.importorskip("sklearn.base")
    p = est.get_params()
    assert type(est)(**p).get_params() == p
    assert est.set_params(**p) is est
    with pytest.raises(ValueError):
        est.set_params(bogus=1)
    est.reference_ = est.covmeans_ = np.eye(2)                      # fitted state must not be copied
    twin = base.clone(est)
    assert twin is not est and twin.get_params() == p
    assert not hasattr(twin, "reference_") and not hasattr(twin, "covmeans_")
    assert repr(twin).startswith(type(est).__name__ + "(")


def test_pipelines_assemble_and_clone():
    pipe = pytest.importorskip("sklearn.pipeline")
    base = pytest.importorskip("sklearn.base")
    lm = pytest.importorskip("sklearn.linear_model")
    clf = pipe.make_pipeline(rm.Covariances(), rm.TangentSpace(), lm.LogisticRegression())
    mdm = pipe.make_pipeline(rm.Covariances(), rm.MDM())
    assert base.is_classifier(mdm) and base.is_classifier(clf)
    for p in (clf, mdm):
        assert base.clone(p).get_params(deep=False).keys() == p.get_params(deep=False).keys()


# ----------------------------------------------------------------------------------------- argument handling
C8 = np.stack([np.eye(8)] * 6)
Y6 = np.array([0, 1, 0, 1, 0, 1])


@pytest.mark.parametrize("make,args", [
    (lambda: rm.Covariances(estimator="lwf"), (np.zeros((6, 8, 16)),)),
    (lambda: rm.Covariances(estimator="oas"), (np.zeros((6, 8, 16)),)),
    (lambda: rm.TangentSpace(metric="logeuclid"), (C8,)),
    (lambda: rm.TangentSpace(tsupdate=True), (C8,)),
    (lambda: rm.MDM(metric="logeuclid"), (C8, Y6)),
    (lambda: rm.MDM(metric={"mean": "riemann", "distance": "wasserstein"}), (C8, Y6)),
    (lambda: rm.TangentSpace(), (np.zeros((2, 129, 129)),)),                    # beyond the 128-channel envelope
])
def test_unprovided_options_raise_not_implemented(make, args):
    est = make()
    with pytest.raises(NotImplementedError):
        est.fit(*args).transform(args[0]) if isinstance(est, rm.Covariances) else est.fit(*args)


@pytest.mark.parametrize("call", [
    lambda: rm.TangentSpace().fit(np.zeros((6, 8, 7))),                          # not square
    lambda: rm.TangentSpace().fit(np.zeros((8, 8))),
    lambda: rm.MDM().fit(C8, Y6[:5]),                                            # mismatched lengths
    lambda: rm.MDM().fit(C8, Y6[:, None]),
    lambda: rm.MDM().fit(C8[0], Y6),
    lambda: rm.Covariances().transform(np.zeros((8, 16))),
    lambda: rm.spd_function(torch.zeros(2, 3, 3), "cube"),
    lambda: rm.spd_function(torch.zeros(2, 3, 3), "log", out="lower"),
])
def test_bad_arguments_raise_value_error(call):
    with pytest.raises(ValueError):
        call()


@pytest.mark.parametrize("call", [
    lambda: rm.spd_function(torch.zeros(2, 3, 3), "log"),                        # a CPU tensor: no CPU fallback
    lambda: rm.spd_eigvalsh(np.zeros((2, 3, 3))),
    lambda: rm.congruence(torch.zeros(2, 3, 3), np.eye(3)),
    lambda: rm.MDM().fit(torch.zeros(6, 8, 8), Y6),
    lambda: rm.TangentSpace().fit(C8.astype(np.int64)),
    lambda: rm.Covariances().transform(np.zeros((6, 8, 16), dtype=np.int32)),
])
def test_wrong_kinds_raise_type_error(call):
    with pytest.raises(TypeError):
        call()


def test_not_fitted():
    for call in (lambda: rm.TangentSpace().transform(C8), lambda: rm.TangentSpace().inverse_transform(np.zeros((2, 36))),
                 lambda: rm.MDM().predict(C8), lambda: rm.MDM().transform(C8), lambda: rm.MDM().predict_proba(C8)):
        with pytest.raises(isd_amd.NotFittedError):
            call()


def test_fitted_state_checks_channels_and_inverse_transform_round_trip():
    ts = rm.TangentSpace()
    covs = spd_stack(5, 6, 3)
    ts.reference_ = ref.mean_riemann(covs)[0]                       # as fit leaves it
    with pytest.raises(ValueError, match="channels"):
        ts.transform(np.stack([np.eye(7)] * 2))
    with pytest.raises(ValueError):
        ts.inverse_transform(np.zeros((2, 20)))
    back = ts.inverse_transform(ref.tangent_space(covs, ts.reference_))          # host-only: exp of the restatement's log
    assert back.shape == covs.shape and np.abs(back - covs).max() <= 1e-12 * np.abs(covs).max()
    mdm = rm.MDM()
    mdm.covmeans_, mdm.classes_ = np.stack([np.eye(6)] * 2), np.array([0, 1])
    with pytest.raises(ValueError, match="channels"):
        mdm.predict(np.stack([np.eye(7)] * 2))


# ------------------------------------------------------------------------------- the restatement checks itself
def test_ref_mean_is_affine_invariant():
    covs = spd_stack(7, 6, 11)
    W = np.random.default_rng(5).standard_normal((6, 6)) + 2 * np.eye(6)
    M, _ = ref.mean_riemann(covs, tol=1e-12)
    Mw, _ = ref.mean_riemann(np.array([W @ c @ W.T for c in covs]), tol=1e-12)
    assert np.abs(Mw - W @ M @ W.T).max() <= 1e-10 * np.abs(Mw).max()


def test_ref_tangent_norm_is_the_distance():
    covs = spd_stack(6, 9, 12)
    M, _ = ref.mean_riemann(covs)
    t = ref.tangent_space(covs, M)
    d = ref.distances(covs, [M])[:, 0]
    assert t.shape == (6, 45)
    assert np.abs(np.linalg.norm(t, axis=1) - d).max() <= 1e-12 * d.max()


def test_ref_mean_of_two_is_the_closed_form():
    A, B = spd_stack(2, 8, 13)
    M, k = ref.mean_riemann(np.array([A, B]), tol=1e-12)
    G = ref.two_matrix_mean(A, B)
    assert k < 50 and np.abs(M - G).max() <= 1e-10 * np.abs(G).max()
    assert abs(ref.distance(A, G) - ref.distance(B, G)) <= 1e-10 * ref.distance(A, B)


def test_ref_three_class_data_leaves_no_trial_inside_the_margin():
    """The MDM test on the GPU compares predictions on every trial whose reference margin exceeds 1e-6 and asserts
    that none is excluded: that is a property of the data, checked here without a GPU."""
    X, y = ref.three_class_trials()
    covs = ref.covariances(X)
    _, means, _ = ref.class_means(covs, y)
    d = np.sort(ref.distances(covs, means), axis=1)
    assert (d[:, 1] - d[:, 0]).min() > 1e-6
    assert np.mean(np.argmin(ref.distances(covs, means), axis=1) == y) > 0.9
