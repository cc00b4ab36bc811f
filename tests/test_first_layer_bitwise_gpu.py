"""GPU: one isd_featcnn_step bit for bit against what it computed before conv5_fwd_glds_kernel and
conv5_wgrad_wide_kernel (csrc/conv.hip) got their explicit fragment prefetch.

tests/golden/first_layer_bitwise.npz holds the raw bits of the first-layer output A2, logits, loss and the flat
gradient for seeded inputs at (B, cin) = (19, 64), (37, 68) and (64, 576) (tools/make_first_layer_golden.py made them
on the GPU; the 576-channel gradient is kept as a SHA-256).  Changes that only move loads and waits around the MFMAs
must reproduce every bit.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_first_layer_golden as mk  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "first_layer_bitwise.npz")


@pytest.fixture(scope="module")
def isd():
    import torch
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd


@pytest.mark.parametrize("name", sorted(mk.CASES))
def test_first_layer_step_bitwise(isd, name):
    golden = np.load(GOLDEN)
    got = mk.run_case(isd, mk.CASES[name])
    for k in ("a2", "logits", "loss", "grad"):
        want = golden[f"{name}.{k}"]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, k
        diff = int((got[k] != want).sum())
        assert diff == 0, f"{name}.{k}: {diff} of {want.size} values differ"
