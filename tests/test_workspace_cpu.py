"""Workspace sizes are behaviour: every size query that needs no device, and the blocks isd_eegnet_sync_block /
isd_paperhead_sync_block hand out, answer what tests/golden/workspace_sizes.json recorded before the layouts moved to
one carved `*_layout` function per call (tools/make_workspace_golden.py asks the questions; the grid is its).  The launch
addresses exactly what the query counts, so an answer that moves is either a wasted or a missing byte."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_workspace_golden as mk  # noqa: E402

QUERIES = ("isd_linear_workspace_bytes", "isd_softmax_ce_workspace_bytes", "isd_pac_work_bytes",
           "isd_envcorr_work_bytes", "isd_ica_step_work_bytes", "isd_tail_fused_save_floats",
           "isd_tail_fused_workspace_floats", "isd_eegnet_workspace_bytes", "isd_paperhead_workspace_bytes",
           "isd_tsception_workspace_bytes", "isd_eegnet_sync_block", "isd_paperhead_sync_block")


def differences(got, want):
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))[:10]
    return {k: (got[k], want[k]) for k in want if got[k] != want[k]}


def test_size_queries_answer_what_they_answered_before():
    import __graft_entry__
    __graft_entry__.build()
    from isd_amd import _lib
    want = json.load(open(mk.GOLDEN))["cpu"]
    got = mk.cpu_cases(_lib.lib())
    bad = differences(got, want)
    assert not bad, (len(bad), dict(list(bad.items())[:10]))


def test_golden_grid_covers_every_query_and_its_refusals():
    want = json.load(open(mk.GOLDEN))["cpu"]
    for name in QUERIES:
        answers = [v for k, v in want.items() if re.match(re.escape(name) + r"\(", k)]
        sizes = [a for a in answers if not isinstance(a, list)]
        assert len(answers) >= 5, name
        if sizes:                                                # a size query: accepted shapes, and refused ones
            assert any(a > 0 for a in sizes) and any(a < 0 for a in sizes), name
            assert all(a in (-1, -2) for a in sizes if a < 0), name
        else:                                                    # a sync block: [rc, byte offset, 8-byte words]
            assert all(a[0] == 0 and a[1] >= 0 and a[1] % 8 == 0 and a[2] > 0 for a in answers), name
    assert want["isd_pac_work_bytes(1, 1, 1, 4097, 0)"] == -2     # past the envelope, not malformed
