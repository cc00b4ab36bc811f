"""Forward extraction vs its input gradient (isd_features_backward), alternating in one process, device events after
warm-up.  cfg2: B = 4096, 64 x 512, 9 bands; cfg5: B = 2048, 128 x 4096 @ 1024 Hz, 40 bands, 1024/960.
Prints one JSON line per configuration (median of the alternating repeats)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import isd_amd

CONFIGS = {
    "cfg2": dict(B=4096, C=64, T=512, fs=256.0, bands=isd_amd.BANDS_9, nperseg=64, noverlap=32),
    "cfg5": dict(B=2048, C=128, T=4096, fs=1024.0, bands=isd_amd.BANDS_40, nperseg=1024, noverlap=960),
}


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2,cfg5")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=0, help="override B (0: the configuration's)")
    a = ap.parse_args()
    for name in a.configs.split(","):
        c = dict(CONFIGS[name])
        if a.batch:
            c["B"] = a.batch
        fx = isd_amd.FeatureExtractor(c["T"], c["fs"], c["bands"], nperseg=c["nperseg"], noverlap=c["noverlap"])
        x = torch.randn(c["B"], c["C"], c["T"], device="cuda")
        out = torch.empty(c["B"], fx.n_bands, c["C"], fx.n_frames, device="cuda")
        g = torch.randn_like(out)
        fwd = lambda: fx(x, out=out)
        bwd = lambda: fx.backward(x, g)
        for _ in range(a.warmup):
            fwd()
            bwd()
        torch.cuda.synchronize()
        tf, tb = [], []
        for _ in range(a.repeats):
            tf.append(timed(fwd, a.iters))
            tb.append(timed(bwd, a.iters))
        tf.sort()
        tb.sort()
        mf, mb = tf[len(tf) // 2], tb[len(tb) // 2]
        print(json.dumps({"config": name, "B": c["B"], "fused": fx.can_fuse, "precision": fx.fb.precision,
                          "forward_ms": round(mf, 4), "backward_ms": round(mb, 4), "ratio": round(mb / mf, 2),
                          "forward_ms_all": [round(v, 4) for v in tf], "backward_ms_all": [round(v, 4) for v in tb]}),
              flush=True)


if __name__ == "__main__":
    main()
