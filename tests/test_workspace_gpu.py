"""GPU: the workspace sizes whose plan lives on the device -- Welch PSD / CSD, the conv stack on each of its routes, the
extractor's backward -- against tests/golden/workspace_sizes.json (tools/make_workspace_golden.py --gpu recorded them
before the layouts moved to one carved `*_layout` function per call).  Plans are created; nothing is launched."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_workspace_golden as mk  # noqa: E402


def test_device_plan_size_queries_answer_what_they_answered_before():
    import torch
    from isd_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    h = _lib.lib()
    want = json.load(open(mk.GOLDEN))["gpu"]
    chunk = h.isd_csd_chunk_bytes(-1)
    got = mk.gpu_cases(h)
    assert h.isd_csd_chunk_bytes(-1) == chunk                    # the chunk setting is back where it was
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))[:10]
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, (len(bad), dict(list(bad.items())[:10]))
    assert all(v > 0 for v in want.values()) and len(want) >= 40
    for over, f64 in ((0, 0), (0, 1), (1, 0), (1, 1)):           # three chunks of one trial need less than four trials at once
        assert want[f"isd_csd_work_bytes[chunk=60000](3, 8, 1024, {over}, {f64})"] < \
            want[f"isd_csd_work_bytes(4, 8, 1024, {over}, {f64})"]
