"""GPU: one isd_featcnn_step bit for bit against what it computed before conv5_wgrad_wide_kernel (csrc/conv.hip) got
its compile-time-stage instances <GT, 13>, which run a full stage (four items of 13 output steps) as straight-line
code and a ragged stage in the generic loop.  The cases are the smallest batches at 576 channels (nine channel groups,
the dbias wave only in the first) whose workgroups run one full stage and a ragged one of 1, 2 and 3 items, two full
stages and a ragged one, a ragged stage alone (a last workgroup of one item) and full stages alone (a last workgroup
of 8 items); and one at 128 channels whose workgroups never have a full stage.

tests/golden/first_layer_wgrad_stage_bitwise.npz holds A2 (SHA-256), logits, loss (raw bits) and the flat gradient
(SHA-256) that the commit before the change computed (tools/make_first_layer_wgrad_stage_golden.py made them on the
GPU).  Every accumulator sees the same operands in the same order, so every bit must come back.  Each case asserts the
kernels (isd_first_layer_last_path) and the stage loop (isd_first_wgrad_last_stage_loop) that ran; 16-sample rows
(12 output steps) must stay on the generic loop.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_first_layer_wgrad_stage_golden as mk  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "first_layer_wgrad_stage_bitwise.npz")


@pytest.fixture(scope="module")
def isd():
    import torch
    import isd_amd
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return isd_amd


@pytest.mark.parametrize("name", sorted(mk.CASES))
def test_first_layer_wgrad_stage_bitwise(isd, name):
    golden = np.load(GOLDEN)
    case = mk.CASES[name]
    got = mk.run_case(isd, case)
    assert got["path"] == (case[3], mk.WGRAD_WIDE), f"{name}: first-layer kernels {got['path']}"
    assert got["loop"] == mk.LOOP_STAGES, f"{name}: stage loop {got['loop']}"
    for k in mk.KEYS:
        want = golden[f"{name}.{k}"]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, k
        diff = int((got[k] != want).sum())
        assert diff == 0, f"{name}.{k}: {diff} of {want.size} values differ"


def test_twelve_output_steps_keep_the_generic_loop(isd):
    """16-sample rows: 12 output steps, so the wide weight gradient runs, on its generic stage loop (its numbers are
    the existing suite's: tests/test_conv_gpu.py, tests/test_classifier_gpu.py)."""
    import torch
    from isd_amd import _lib
    from isd_amd.classifier import _FeatureModel
    B, cin, W = 64, 128, 16
    torch.manual_seed(46)
    m = _FeatureModel(cin, mk.staging.F, mk.staging.N_CLS, 4).cuda()
    x = torch.randn(B, cin, W, device="cuda")
    y = torch.randint(0, mk.staging.N_CLS, (B,), device="cuda")
    assert _lib.lib().isd_featcnn_supported(m.conv_plan(x)._h, B, W, mk.staging.N_CLS) == 1
    isd.HotPath(m).forward(x, y, want_grad=True)
    torch.cuda.synchronize()
    assert mk.staging.last_path()[1] == mk.WGRAD_WIDE
    assert mk.stage_loop() == mk.LOOP_GENERIC
    assert bool(torch.isfinite(m.flat_grads()).all())

