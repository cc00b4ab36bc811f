"""Write tests/golden/first_layer_bitwise.npz: what one isd_featcnn_step (fp32, one zone, 32 filters, 17-sample rows)
computes for seeded inputs at (B, cin) = (19, 64), (37, 68) and (64, 576) -- the first-layer output A2, logits, loss
and the flat gradient, as raw bits.  The first layer runs on conv5_fwd_glds_kernel and conv5_wgrad_wide_kernel
(csrc/conv.hip); tests/test_first_layer_bitwise_gpu.py recomputes every case and compares bit for bit, so changes
that only move those kernels' loads and waits around their MFMAs must reproduce the file.

The committed file was made by commit 523d159 ("Run the fp32 classifier tail at two waves per SIMD"), the last one
before the two kernels got their explicit fragment prefetch.

The gradient at 576 channels (2.4 MB) is kept as its SHA-256: a committed file stays below 1 MiB.

Needs a GPU.  Run it from the commit whose kernels the test pins:
    python tools/make_first_layer_golden.py [OUT.npz]
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

F, N_CLS, W = 32, 5, 17
GRAD_DIGEST_ABOVE = 100_000          # gradients longer than this are stored as a digest

# name: (B, cin, seed)
CASES = {
    "b19_c64": (19, 64, 21),
    "b37_c68": (37, 68, 22),
    "b64_c576": (64, 576, 23),
}


def a2_offset(cin):
    """Float offset of A2 in the conv4 workspace of a one-zone, 32-filter plan (make_geo in csrc/conv.hip: the Weff
    fragments chunk-aligned to 32 channels, their bf16 twin, beff, then cnn3 / cnn4 and their transposes)."""
    def up(n, m):
        return (n + m - 1) // m * m
    gt = F // 16
    eff = up(cin, 32) // 4 * 5 * gt * 64
    conv = up((F // 4) * 5 * gt * 64, 64)
    return up(eff, 64) + up(eff // 5 * 4, 64) + up(F, 64) + 4 * conv


def inputs(B, cin, seed):
    """Parameters (flat block of _FeatureModel(cin, 32, 5, 4)), features and labels of a case."""
    rng = np.random.default_rng(seed)
    n_params = F * 5 + F + F * F * cin + 2 * F * F * 5 + N_CLS * F + N_CLS
    theta = (rng.standard_normal(n_params) * 0.05).astype(np.float32)
    x = rng.standard_normal((B, cin, W)).astype(np.float32)
    y = rng.integers(0, N_CLS, B).astype(np.int64)
    return theta, x, y


def bits(t):
    import torch
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32).copy()


def digest(u32):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(u32).tobytes()).digest(), dtype=np.uint8).copy()


def run_case(isd, case):
    """dict(a2, logits, loss, grad) of the case as uint32 bit patterns (grad as a SHA-256 when it is long)."""
    import torch
    from isd_amd import _lib
    from isd_amd.classifier import _FeatureModel
    B, cin, seed = case
    theta, x, y = inputs(B, cin, seed)
    m = _FeatureModel(cin, F, N_CLS, 4).cuda()
    flat = m.flat_params()
    assert flat.numel() == theta.size, (flat.numel(), theta.size)
    flat.copy_(torch.from_numpy(theta))
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    assert _lib.lib().isd_featcnn_supported(m.conv_plan(xd)._h, B, W, N_CLS) == 1
    hp = isd.HotPath(m)
    out = hp.forward(xd, yd, want_grad=True)
    torch.cuda.synchronize()
    n_a2 = B * F * (W - 4)
    o = a2_offset(cin)
    grad = bits(m.flat_grads())
    return {"a2": bits(hp._ws["conv"][o:o + n_a2]), "logits": bits(out["logits"]), "loss": bits(out["loss"].reshape(1)),
            "grad": digest(grad) if grad.size > GRAD_DIGEST_ABOVE else grad}


def main():
    import isd_amd
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "first_layer_bitwise.npz")
    arrays = {}
    for name, case in CASES.items():
        for k, v in run_case(isd_amd, case).items():
            arrays[f"{name}.{k}"] = v
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print(out, {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
