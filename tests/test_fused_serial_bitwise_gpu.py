"""GPU: fused_serial_kernel (csrc/fb.hip) bit for bit against maps it computed before its instruction-level rework.

tests/golden/fused_serial_bitwise.npz holds the raw bits of the maps of every kernel instance -- bands per wave 1 / 2 / 3,
log-power / power / magnitude, the fp32 and the bf16 map -- for seeded inputs (tools/make_fused_serial_golden.py made
them on the GPU).  Changes that only move instructions around the arithmetic must reproduce every bit.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_fused_serial_golden as mk  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "fused_serial_bitwise.npz")


@pytest.fixture(scope="module")
def isd():
    import torch
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd


@pytest.mark.parametrize("name", sorted(mk.CASES))
def test_fused_serial_kernel_bitwise(isd, name):
    want = np.load(GOLDEN)[name]
    got, path = mk.run_case(isd, mk.CASES[name])
    assert path == 2, path                                # fused_serial_kernel ran, not a fall-back
    assert got.dtype == want.dtype and got.shape == want.shape
    diff = int((got != want).sum())
    assert diff == 0, f"{name}: {diff} of {got.size} values differ"
