"""GPU: the flat layout of the one-row-per-lane extractor (csrc/fb.hip, fused_serial_kernel<0, MAG>: one band per wave,
(row group, band) slots numbered across workgroups of 16 or 8 waves) against the grouped layout it replaces as the
default, bit for bit.

Both layouts run the same chunk body, so every value of the map -- fp32 or bf16 -- must be equal, whatever the slot
mapping does: row groups split between two workgroups, a ragged last row group, waves whose slot lies past the end, one
to four tiles per workgroup.  The grouped side is pinned with ISD_SERIAL_BPW=1; isd_features_fused_last_serial_waves()
tells which layout a call took (16 / 8 flat, 0 grouped), so neither side can pass by running the other's kernel.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

from oracle import dsp as odsp
from test_features_gpu import TOL_FEAT

pytestmark = pytest.mark.gpu

_KEYS = ("ISD_FUSED_SERIAL", "ISD_SERIAL_BPW", "ISD_SERIAL_GROUPS", "ISD_SERIAL_FLAT")
BANDS_12 = tuple(odsp.BANDS_9) + (("x1", 10.0, 14.0), ("x2", 18.0, 22.0), ("x3", 26.0, 30.0))   # make_fused_serial_golden.py


@pytest.fixture(scope="module")
def isd():
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in _KEYS}
    for k in _KEYS:
        os.environ.pop(k, None)
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(fx, x, bf16=False, **env):
    """The map as raw bits, the family and the flat layout's waves per workgroup of the call."""
    from isd_amd import _lib
    with _env(**env):
        out = fx(x, fused=True, out_dtype=torch.bfloat16 if bf16 else torch.float32)
        torch.cuda.synchronize()
        path = int(_lib.lib().isd_features_fused_last_path())
        waves = int(_lib.lib().isd_features_fused_last_serial_waves())
    return out.view(torch.int16 if bf16 else torch.int32).cpu().numpy(), path, waves


def _inputs(B, C, T):
    return np.random.default_rng(1000 * B + 10 * C + T).standard_normal((B, C, T)).astype(np.float32)


DEFAULT_WAVES = 8                                         # what the library takes when ISD_SERIAL_FLAT is unset


def _flat_equals_grouped(isd, B, C, T, bands, mode="logpower", bf16=False, flat=16):
    """flat: ISD_SERIAL_FLAT of the flat side; None leaves it unset (the default route)."""
    x = torch.from_numpy(_inputs(B, C, T)).cuda()
    fx = isd.FeatureExtractor(T, 256.0, bands, mode=mode)
    assert fx.fb.precision == "f32"
    env = {} if flat is None else {"ISD_SERIAL_FLAT": str(flat)}
    got, pg, wg = _run(fx, x, bf16, **env)
    want, pw, ww = _run(fx, x, bf16, ISD_SERIAL_BPW="1")
    assert (pg, wg) == (2, DEFAULT_WAVES if flat is None else flat), (pg, wg)   # the flat layout ran ...
    assert (pw, ww) == (2, 0), (pw, ww)                   # ... against the grouped one
    assert got.shape == want.shape == (B, len(bands), C, T // 32 + 1)
    diff = int((got != want).sum())
    assert diff == 0, f"{diff} of {got.size} values differ"
    off, po, wo = _run(fx, x, bf16, ISD_SERIAL_FLAT="0")  # the switch: the grouped default, the same map again
    assert (po, wo) == (2, 0) and np.array_equal(off, want)


# R = 135 rows: three row groups, the last of 7 rows; 27 slots: two workgroups of 16 waves, the second with 11 live
# ones; row group 1 split between them.  Five chunks: the closing frame takes the ragged store path.
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("mode", ["logpower", "power", "magnitude"])
def test_flat_equals_grouped_every_mode_and_map(isd, mode, bf16):
    _flat_equals_grouped(isd, 27, 5, 160, odsp.BANDS_9, mode=mode, bf16=bf16)


@pytest.mark.parametrize("B,C,T,bands,bf16", [
    (27, 5, 32, odsp.BANDS_9, False),                     # one chunk, J = 2
    (2, 64, 512, odsp.BANDS_9, False),                    # the headline row
    (2, 64, 512, odsp.BANDS_9, True),
    (1, 9, 256, BANDS_12, False),                         # 12 bands, 9 rows: one workgroup, four dead waves
    (7, 64, 96, odsp.BANDS_9[2:7], False),                # 5 bands, 7 row groups: slots 16..31 touch four tiles (64 KiB)
])
def test_flat_equals_grouped_over_the_slot_mapping(isd, B, C, T, bands, bf16):
    _flat_equals_grouped(isd, B, C, T, bands, bf16=bf16)


def test_flat_with_eight_waves_per_workgroup(isd):
    _flat_equals_grouped(isd, 27, 5, 160, odsp.BANDS_9, flat=8)


def test_default_route_of_nine_bands(isd):
    _flat_equals_grouped(isd, 27, 5, 160, odsp.BANDS_9, flat=None)


@pytest.mark.parametrize("nb,flat", [(4, "16"), (2, None)])
def test_plans_whose_tiles_do_not_fit_keep_the_grouped_layout(isd, nb, flat):
    """Four bands at 16 waves: ceil(15 / 4) + 1 = 5 tiles; two bands at the default 8 waves: ceil(7 / 2) + 1 = 5.  More
    than the four tiles a workgroup may hold, so the route stays grouped and computes what ISD_SERIAL_BPW=1 does."""
    bands = odsp.BANDS_9[:nb]
    x = torch.from_numpy(_inputs(27, 5, 160)).cuda()
    fx = isd.FeatureExtractor(160, 256.0, bands)
    got, p, w = _run(fx, x, **({} if flat is None else {"ISD_SERIAL_FLAT": flat}))
    want, pw, ww = _run(fx, x, ISD_SERIAL_BPW="1")
    assert (p, w) == (2, 0) and (pw, ww) == (2, 0)
    assert np.array_equal(got, want)


def test_flat_against_the_oracle(isd):
    X = _inputs(27, 5, 160)
    fx = isd.FeatureExtractor(160, 256.0, odsp.BANDS_9)
    got, p, w = _run(fx, torch.from_numpy(X).cuda(), ISD_SERIAL_FLAT="16")
    assert (p, w) == (2, 16)
    ref = odsp.extract_features_scipy(X, fs=256.0, bands=odsp.BANDS_9).astype(np.float64)
    err = np.abs(got.view(np.float32).astype(np.float64) - ref).max()
    assert err < TOL_FEAT, err
