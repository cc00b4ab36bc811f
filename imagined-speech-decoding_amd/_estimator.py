"""What every estimator of the package shares: the sklearn parameter protocol, the not-fitted error, the sklearn tags
of a transformer, and the handling of [n, C, T] trials that come as an ndarray or as a CUDA tensor.  The classical
transformers (csp, fbcsp, ica, riemann) and the trained classifiers (classifier) all build on it, and it builds on
``_lib`` alone.
"""
import numpy as np
import torch

from . import _lib


class NotFittedError(ValueError, AttributeError):
    """Same base classes as ``sklearn.exceptions.NotFittedError`` (raised by predict / transform before fit)."""


class Estimator:
    """sklearn estimator protocol: constructor arguments are stored verbatim under their own names, listed in
    ``_param_names`` (``get_params`` / ``set_params`` / ``sklearn.base.clone`` work); fitted state lives in
    trailing-underscore attributes."""
    _param_names = ()

    def get_params(self, deep=True):
        return {k: getattr(self, k) for k in self._param_names}

    def set_params(self, **params):
        for k, v in params.items():
            if k not in self._param_names:
                raise ValueError(f"invalid parameter {k!r} for {type(self).__name__}")
            setattr(self, k, v)
        return self

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={getattr(self, k)!r}' for k in self._param_names)})"

    def _require_fitted(self, attr, how):
        """Raises unless fit has left ``attr``; ``how`` finishes the sentence 'call ...'."""
        if getattr(self, attr, None) is None:
            raise NotFittedError(f"this {type(self).__name__} instance is not fitted yet: call {how}")


def transformer_tags(required_y, requires_fit=True):
    """The ``__sklearn_tags__`` of a transformer of [n, C, T] or [n, C, C] arrays.  Called by sklearn only (Pipeline,
    clone, checks), so sklearn is imported here and nowhere else."""
    from sklearn.utils import InputTags, Tags, TargetTags, TransformerTags
    return Tags(estimator_type=None, target_tags=TargetTags(required=required_y), transformer_tags=TransformerTags(),
                input_tags=InputTags(three_d_array=True), requires_fit=requires_fit)


def check_trials(X, dtypes=(torch.float32, torch.float64)):
    """X [n, C, T] as ``_lib.check_array`` leaves it: a CUDA tensor of one of ``dtypes``, or a float ndarray."""
    X, _ = _lib.check_array(X, "X", dtypes)
    if X.ndim != 3:
        raise ValueError(f"X must be [n, C, T], got {tuple(X.shape)}")
    return X


def chunks(X, rows, who, dtype=np.float64):
    """(start, CUDA [<= rows, C, T] slice) of X in order; an ndarray is uploaded slice by slice as ``dtype``."""
    is_tensor = isinstance(X, torch.Tensor)
    for s in range(0, X.shape[0], rows):
        yield s, _lib.to_device(X[s:s + rows], is_tensor, who, dtype)


def like(res, X):
    """A CUDA result in X's kind: CUDA tensor -> tensor of X's dtype, ndarray -> float64 ndarray."""
    return res.to(X.dtype) if isinstance(X, torch.Tensor) else res.double().cpu().numpy()


def cat_like(parts, X, tail):
    """The per-chunk results joined along the trials, in X's kind; [0, *tail] when X has no trial."""
    if parts:
        return like(torch.cat(parts), X)
    if isinstance(X, torch.Tensor):
        return torch.empty(0, *tail, dtype=X.dtype, device=X.device)
    return np.empty((0, *tail))
