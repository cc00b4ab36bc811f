"""Write tests/golden/first_layer_staging_bitwise.npz: what one isd_featcnn_step (fp32, one zone, 32 filters, 17-sample
rows) computes for seeded inputs at the smallest batches that reach the parts of the first-layer kernels' LDS-DMA
staging which tests/golden/first_layer_bitwise.npz does not: conv5_fwd_glds_kernel<2, 2> (several items per wave,
waves with unequal item counts, a last workgroup with one item), conv5_fwd_glds_kernel<2, 4> with 6 and 9 items per
workgroup, and conv5_wgrad_wide_kernel with ragged last stages and a second channel group of 4 rows.
tests/test_first_layer_staging_gpu.py recomputes every case and compares bit for bit, so a change that only alters how
the DMA of those kernels is issued must reproduce the file.

The committed file was made by commit ade8b95 ("Add a GPU FastICA transformer for artifact removal"), the last one
before the staging of the two kernels was issued as straight-line code.

A2 (up to 3.8 MB a case) is kept as the SHA-256 of its bytes, and so is a gradient of more than 100 000 values
(cin = 128) and every gradient but that of the 68-channel case: the six raw gradients are 2.4 MB, and a committed file
stays below 1 MiB.  Logits and loss are raw bits.

Needs a GPU.  Run it from the commit whose kernels the test pins:
    python tools/make_first_layer_staging_golden.py [OUT.npz]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import make_first_layer_golden as base  # noqa: E402

F, N_CLS, W = base.F, base.N_CLS, base.W

# isd_first_layer_last_path(): forward instance + 16 * weight-gradient kernel
FWD_GLDS_2_2, FWD_GLDS_2_4, WGRAD_WIDE = 1, 2, 1

# name: (B, cin, seed, forward instance, raw gradient)
#   b2305: ceil(2305 / 9) = 257 workgroups > 256 -> <2, 2>, 9 items per workgroup (wave 0 stages 3, the others 2), the
#          last workgroup has one item; cin = 68: two full chunks and a ragged one, second wgrad channel group of 4 rows
#   b1300: <2, 4>, 6 items per workgroup, the last has 4;  b2304: <2, 4>, 9 items per workgroup
#   b19 / b37 at 128 channels: two full channel groups in the weight gradient, item ranges that are no multiple of
#          the 4 items of a stage
CASES = {
    "b2305_c64": (2305, 64, 31, FWD_GLDS_2_2, False),
    "b2305_c68": (2305, 68, 32, FWD_GLDS_2_2, True),
    "b1300_c64": (1300, 64, 33, FWD_GLDS_2_4, False),
    "b2304_c64": (2304, 64, 34, FWD_GLDS_2_4, False),
    "b19_c128": (19, 128, 35, FWD_GLDS_2_4, False),
    "b37_c128": (37, 128, 36, FWD_GLDS_2_4, False),
}
KEYS = ("a2", "logits", "loss", "grad")


def last_path():
    """(forward instance, weight-gradient kernel) of the last first-layer launches, or None from a library that
    predates isd_first_layer_last_path (the commit that made the golden file)."""
    from isd_amd import _lib
    fn = getattr(_lib.lib(), "isd_first_layer_last_path", None)
    if fn is None:
        return None
    v = int(fn())
    return v & 15, v >> 4


def run_case(isd, case):
    """dict(a2, logits, loss, grad, path) of the case: uint32 bit patterns or their SHA-256, and last_path()."""
    import torch
    from isd_amd import _lib
    from isd_amd.classifier import _FeatureModel
    B, cin, seed, _, raw_grad = case
    theta, x, y = base.inputs(B, cin, seed)
    m = _FeatureModel(cin, F, N_CLS, 4).cuda()
    flat = m.flat_params()
    assert flat.numel() == theta.size, (flat.numel(), theta.size)
    flat.copy_(torch.from_numpy(theta))
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    assert _lib.lib().isd_featcnn_supported(m.conv_plan(xd)._h, B, W, N_CLS) == 1
    hp = isd.HotPath(m)
    out = hp.forward(xd, yd, want_grad=True)
    torch.cuda.synchronize()
    path = last_path()
    n_a2 = B * F * (W - 4)
    o = base.a2_offset(cin)
    grad = base.bits(m.flat_grads())
    return {"a2": base.digest(base.bits(hp._ws["conv"][o:o + n_a2])), "logits": base.bits(out["logits"]),
            "loss": base.bits(out["loss"].reshape(1)), "grad": grad if raw_grad else base.digest(grad), "path": path}


def main():
    import isd_amd
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "first_layer_staging_bitwise.npz")
    arrays = {}
    for name, case in CASES.items():
        got = run_case(isd_amd, case)
        for k in KEYS:
            arrays[f"{name}.{k}"] = got[k]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print(out, {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
