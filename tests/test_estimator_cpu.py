"""The estimator protocol every estimator of the package inherits (isd_amd/_estimator.py) and the precision dispatch
of the library binding (``_lib.typed``).  No GPU, no library."""
import types

import pytest
import torch

import isd_amd
from isd_amd import _estimator, _lib, classifier, riemann

ESTIMATORS = [isd_amd.CSP, isd_amd.FBCSP, isd_amd.ICA, riemann.Covariances, riemann.CoSpectra, riemann.TangentSpace,
              riemann.MDM, isd_amd.FilterbankCNNClassifier, isd_amd.FilterbankEEGNetClassifier,
              isd_amd.FASTHeadClassifier, isd_amd.TSceptionClassifier]


@pytest.mark.parametrize("cls", ESTIMATORS, ids=lambda c: c.__name__)
def test_protocol_is_inherited_not_restated(cls):
    assert issubclass(cls, _estimator.Estimator)
    for klass in cls.__mro__:
        if klass not in (_estimator.Estimator, object):
            assert not {"get_params", "set_params", "__repr__"} & set(vars(klass)), klass


@pytest.mark.parametrize("cls", ESTIMATORS, ids=lambda c: c.__name__)
def test_params_round_trip_and_repr(cls):
    est = cls()
    params = est.get_params()
    assert params and list(params) == list(cls._param_names) and est.get_params(deep=False) == params
    assert cls(**params).get_params() == params
    name = next(iter(params))
    assert est.set_params(**{name: params[name]}) is est and est.get_params() == params
    with pytest.raises(ValueError):
        est.set_params(bogus=1)
    text = repr(est)
    assert text.startswith(cls.__name__ + "(") and text.endswith(")")
    assert all(f"{k}=" in text for k in params)


def test_not_fitted_error_is_one_class():
    assert isd_amd.NotFittedError is classifier.NotFittedError is _estimator.NotFittedError
    assert _estimator.NotFittedError.__bases__ == (ValueError, AttributeError)


def test_require_fitted_names_the_class_and_the_remedy():
    est = isd_amd.CSP()
    with pytest.raises(isd_amd.NotFittedError, match=r"this CSP instance is not fitted yet: call fit\(X\) first"):
        est._require_fitted("filters_", "fit(X) first")
    est.filters_ = None                                             # the classifiers reset model_ to None
    with pytest.raises(isd_amd.NotFittedError):
        est._require_fitted("filters_", "fit(X) first")
    est.filters_ = 0.0
    est._require_fitted("filters_", "fit(X) first")


def test_typed_picks_the_entry_point_of_the_dtype(monkeypatch):
    stand_in = types.SimpleNamespace(isd_thing_f32=object(), isd_thing_f64=object())
    monkeypatch.setattr(_lib, "_lib", stand_in)                     # what lib() returns once loaded: nothing is loaded
    assert _lib.typed("isd_thing", torch.float32) is stand_in.isd_thing_f32
    assert _lib.typed("isd_thing", torch.float64) is stand_in.isd_thing_f64
    with pytest.raises(KeyError):
        _lib.typed("isd_thing", torch.float16)
    with pytest.raises(AttributeError):
        _lib.typed("isd_other", torch.float32)
