"""GPU: one isd_featcnn_step bit for bit against what it computed before the LDS-DMA staging of
conv5_fwd_glds_kernel and conv5_wgrad_wide_kernel (csrc/conv.hip) was issued as straight-line code, at the smallest
batches that stage several items per wave, give the waves unequal item counts, end on a workgroup with fewer items,
mix full and ragged channel chunks, and end a weight-gradient item range on a ragged stage.

tests/golden/first_layer_staging_bitwise.npz holds the first-layer output A2 (SHA-256), logits, loss and the flat
gradient (raw bits or SHA-256) that the commit before the change computed (tools/make_first_layer_staging_golden.py
made them on the GPU).  The staging moves the same bytes to the same LDS addresses and no MFMA changes, so every bit
must come back.  Each case also asserts that the intended kernel instances ran (isd_first_layer_last_path).
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_first_layer_staging_golden as mk  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "first_layer_staging_bitwise.npz")


@pytest.fixture(scope="module")
def isd():
    import torch
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd


@pytest.mark.parametrize("name", sorted(mk.CASES))
def test_first_layer_staging_bitwise(isd, name):
    golden = np.load(GOLDEN)
    case = mk.CASES[name]
    got = mk.run_case(isd, case)
    assert got["path"] == (case[3], mk.WGRAD_WIDE), f"{name}: first-layer kernels {got['path']}"
    for k in mk.KEYS:
        want = golden[f"{name}.{k}"]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, k
        diff = int((got[k] != want).sum())
        assert diff == 0, f"{name}.{k}: {diff} of {want.size} values differ"
