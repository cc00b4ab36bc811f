"""Write tests/golden/first_layer_wgrad_stage_bitwise.npz: what one isd_featcnn_step (fp32, one zone, 32 filters,
17-sample rows) computes for seeded inputs at the smallest batches that mix full and ragged stages of
conv5_wgrad_wide_kernel in every way its compile-time-stage instances (<GT, 13>: a full stage of four 13-step items as
straight-line code, a ragged stage in the generic loop) tell apart.  tests/test_first_layer_wgrad_stage_gpu.py
recomputes every case and compares bit for bit: the instances issue the same reads and MFMAs in the same order, so
every bit must come back.

The committed file was made by commit 128cd93 ("Add Morlet time-frequency transform on the GPU"), the last one before
the instances existed.

A2 and the flat gradient are kept as the SHA-256 of their bytes, logits and loss as raw bits.

Needs a GPU.  Run it from the commit whose kernels the test pins (a library without isd_first_wgrad_last_stage_loop
is fine: the query is only reported, not stored):
    python tools/make_first_layer_wgrad_stage_golden.py [OUT.npz]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import make_first_layer_staging_golden as staging  # noqa: E402

FWD_GLDS_2_4, WGRAD_WIDE = staging.FWD_GLDS_2_4, staging.WGRAD_WIDE
LOOP_GENERIC, LOOP_STAGES = 0, 1        # isd_first_wgrad_last_stage_loop()

# name: (B, cin, seed, forward instance, raw gradient)   -- the tuple of make_first_layer_staging_golden.run_case
#   576 channels: nine channel groups, the dbias wave only in group 0; 768 / 9 = 85 item ranges, so a workgroup has
#   ceil(B / 85) items and a stage four of them:
#   b341: 5 = one full stage + a ragged one of 1; the last of the 69 workgroups has one item, a ragged stage alone
#   b510: 6 = full + ragged 2;   b595: 7 = full + ragged 3
#   b683: 9 = two full + ragged 1; the last of the 76 workgroups has 8 items and ends on a full stage
#   128 channels, b37: one item per workgroup -- the <2, 13> instance never enters its straight-line stage
CASES = {
    "b341_c576": (341, 576, 41, FWD_GLDS_2_4, False),
    "b510_c576": (510, 576, 42, FWD_GLDS_2_4, False),
    "b595_c576": (595, 576, 43, FWD_GLDS_2_4, False),
    "b683_c576": (683, 576, 44, FWD_GLDS_2_4, False),
    "b37_c128": (37, 128, 45, FWD_GLDS_2_4, False),
}
KEYS = staging.KEYS


def stage_loop():
    """isd_first_wgrad_last_stage_loop(), or None from a library that predates it (the commit that made the golden
    file)."""
    from isd_amd import _lib
    fn = getattr(_lib.lib(), "isd_first_wgrad_last_stage_loop", None)
    return None if fn is None else int(fn())


def run_case(isd, case):
    """staging.run_case plus "loop": stage_loop() after the step."""
    got = staging.run_case(isd, case)
    got["loop"] = stage_loop()
    return got


def main():
    import isd_amd
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden",
                                                             "first_layer_wgrad_stage_bitwise.npz")
    arrays = {}
    for name, case in CASES.items():
        got = run_case(isd_amd, case)
        print(name, "path", got["path"], "loop", got["loop"])
        for k in KEYS:
            arrays[f"{name}.{k}"] = got[k]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print(out, {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
