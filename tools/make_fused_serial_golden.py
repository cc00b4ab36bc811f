"""Write tests/golden/fused_serial_bitwise.npz: the feature maps fused_serial_kernel (csrc/fb.hip) computes for small
seeded inputs, one case per kernel instance -- bands per wave 1 / 2 / 3, log-power / power / magnitude (MAG), the fp32
and the bf16 map -- plus the reference-native 800-sample trial and a 12-band plan.
tests/test_fused_serial_bitwise_gpu.py recomputes every case and compares bit for bit.

Needs a GPU.  Run it from the commit whose kernel the test pins:
    python tools/make_fused_serial_golden.py [OUT.npz]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

EXTRA = (("x1", 10.0, 14.0), ("x2", 18.0, 22.0), ("x3", 26.0, 30.0))

# name: (B, C, T, fs, band set, mode, bands per wave, bf16 map, seed)
CASES = {
    "logpower_bpw3": (2, 33, 512, 256.0, "9", "logpower", 3, False, 11),
    "logpower_bpw2": (2, 33, 512, 256.0, "9", "logpower", 2, False, 11),
    "logpower_bpw1": (2, 33, 512, 256.0, "9", "logpower", 1, False, 11),
    "power_bpw2": (2, 33, 512, 256.0, "9", "power", 2, False, 12),
    "magnitude_bpw3": (2, 33, 512, 256.0, "9", "magnitude", 3, False, 13),
    "magnitude_bpw1": (1, 64, 512, 256.0, "9", "magnitude", 1, False, 14),
    "logpower_bf16_bpw3": (2, 33, 512, 256.0, "9", "logpower", 3, True, 11),
    "magnitude_bf16_bpw2": (1, 40, 512, 256.0, "9", "magnitude", 2, True, 15),
    "logpower_t800": (2, 7, 800, 250.0, "9", "logpower", 3, False, 16),
    "logpower_12bands": (1, 9, 256, 256.0, "12", "logpower", 3, False, 17),
}


def bands_of(name):
    from oracle import dsp as odsp
    return tuple(odsp.BANDS_9) if name == "9" else tuple(odsp.BANDS_9) + EXTRA


def inputs(B, C, T, seed):
    return np.random.default_rng(seed).standard_normal((B, C, T)).astype(np.float32)


def run_case(isd, case):
    """The case's map as raw bits (uint32 for fp32, uint16 for bf16) and the kernel family that ran."""
    import torch
    from isd_amd import _lib
    B, C, T, fs, bset, mode, bpw, bf16, seed = case
    keys = ("ISD_FUSED_SERIAL", "ISD_SERIAL_BPW", "ISD_SERIAL_GROUPS")
    old = {k: os.environ.get(k) for k in keys}
    os.environ["ISD_FUSED_SERIAL"], os.environ["ISD_SERIAL_BPW"] = "1", str(bpw)
    os.environ.pop("ISD_SERIAL_GROUPS", None)
    try:
        fx = isd.FeatureExtractor(T, fs, bands_of(bset), mode=mode)
        x = torch.from_numpy(inputs(B, C, T, seed)).cuda()
        out = fx(x, fused=True, out_dtype=torch.bfloat16 if bf16 else torch.float32)
        torch.cuda.synchronize()
        path = int(_lib.lib().isd_features_fused_last_path())
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    bits = out.view(torch.int16 if bf16 else torch.int32).cpu().numpy()
    return bits.view(np.uint16 if bf16 else np.uint32), path


def main():
    import isd_amd
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "fused_serial_bitwise.npz")
    maps = {}
    for name, case in CASES.items():
        bits, path = run_case(isd_amd, case)
        assert path == 2, (name, path)                    # fused_serial_kernel ran
        maps[name] = bits
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **maps)
    print(out, {k: v.shape for k, v in maps.items()})


if __name__ == "__main__":
    main()
