#!/usr/bin/env python3
"""Config 5 (128 ch, 4 s @ 1024 Hz, 40 bands, 1024/960 STFT, EEGNet_Encoder(5120, 32) + Linear(32, 5)) at B = 2048:
the true training step with an fp32 and with a bf16 feature map, A/B in one process.

Each step = one fused extraction of the resident batch into the map + one Trainer step (EEGNet fwd + bwd + Linear +
CE + AdamW) on it, timed with events per stage.  The legs alternate in rounds of --steps steps so that clock drift
hits both alike; every leg has its own model, built from the same seed.  One JSON line per leg (median and min..max
of the per-step stage times over all rounds), then one summary line.

  python tools/bench_cfg5_bf16.py [--batch 2048] [--rounds 6] [--steps 5] [--legs fp32,bf16]

Under `rocprofv3 --kernel-trace --stats` run one leg (`--legs bf16`) for a per-kernel table of that leg alone."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="fp32,bf16")
    a = ap.parse_args()
    import isd_amd
    from isd_amd.classifier import _EEGNetFeatureModel
    B, C, T, fs = a.batch, 128, 4096, 1024.0
    legs = a.legs.split(",")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, C, T, device=dev, generator=gen)
    y = torch.randint(0, 5, (B,), device=dev, generator=gen)
    fx = isd_amd.FeatureExtractor(T, fs, isd_amd.BANDS_40, nperseg=1024, noverlap=960)
    nb, J = fx.n_bands, fx.n_frames
    state = {}
    for leg in legs:
        torch.manual_seed(42)
        model = _EEGNetFeatureModel(nb * C, 32, 5, kernel_length=64, dropout=0.25).to(dev)
        dt = torch.bfloat16 if leg == "bf16" else torch.float32
        state[leg] = dict(tr=isd_amd.Trainer(model, lr=5e-4, weight_decay=1e-2),
                          feat=torch.empty((B, nb, C, J), dtype=dt, device=dev), ext=[], cls=[], tot=[], loss=None)

    def step(s, ev=None):
        if ev:
            ev[0].record()
        fx(x, fused=True, out=s["feat"])
        if ev:
            ev[1].record()
        out = s["tr"].step(s["feat"].view(B, nb * C, J), y)
        if ev:
            ev[2].record()
        return out

    for leg in legs:
        for _ in range(a.warmup):
            step(state[leg])
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for leg in legs:
            s = state[leg]
            evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.steps)]
            for e in evs:
                out = step(s, e)
            torch.cuda.synchronize()
            s["loss"] = float(out["loss"])
            for e in evs:
                s["ext"].append(e[0].elapsed_time(e[1]))
                s["cls"].append(e[1].elapsed_time(e[2]))
                s["tot"].append(e[0].elapsed_time(e[2]))

    def stat(v):
        return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4),
                "max": round(float(np.max(v)), 4)}

    res = {}
    for leg in legs:
        s = state[leg]
        res[leg] = {"leg": leg, "batch": B, "steps": len(s["tot"]), "map_bytes": s["feat"].numel() * s["feat"].element_size(),
                    "extract_ms": stat(s["ext"]), "classifier_ms": stat(s["cls"]), "step_ms": stat(s["tot"]),
                    "trials_per_s": round(B / float(np.median(s["tot"])) * 1e3, 1), "final_loss": s["loss"]}
        print(json.dumps(res[leg]))
    if "fp32" in res and "bf16" in res:
        f, h = res["fp32"], res["bf16"]
        print(json.dumps({"summary": "bf16 - fp32 (medians, ms)",
                          "extract": round(h["extract_ms"]["median"] - f["extract_ms"]["median"], 4),
                          "classifier": round(h["classifier_ms"]["median"] - f["classifier_ms"]["median"], 4),
                          "step": round(h["step_ms"]["median"] - f["step_ms"]["median"], 4)}))


if __name__ == "__main__":
    main()
