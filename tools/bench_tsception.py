"""TSception (csrc/tsception.hip) against the same model in torch ops on the same card and clock.

Shapes: [64, 64, 800] and the notebook's full batch [350, 64, 800] at 250 Hz (``--shapes BxCxT@fs,...`` for others, up
to the model's batch bound of 350 trials per pass: [4096, 64, 512] is refused); num_T = num_S = 15,
hidden 32, five classes.  Per shape one JSON line:
  hip_step / torch_step          training step, forward + backward + AdamW, fp32 (event-timed medians);
  hip_eval / torch_eval          eval-mode forward;
  torch_step_bf16 / torch_eval_bf16   the torch route under bf16 autocast, for information (the notebook's figure was
                                 bf16-mixed); fp32 is the comparison;
  temporal_fwd / temporal_bwd    the temporal stage's kernels alone and their fraction of the fp32 peak (157.3 TFLOP/s),
                                 counting 2 B C num_T sum_s (T - k_s + 1) k_s flops for the forward and twice that for
                                 the backward, which recomputes the pre-activation before it contracts it.
The HIP path and the restatement (tests/tsception_ref.py) alternate inside one process after a warm-up; the shader clock
is probed while the last HIP step is still queued.  Nothing is asserted: where the native step is slower the line says
so (``torch_over_hip_step`` < 1).  ``--hip-only`` runs the HIP step and eval forward alone (for a kernel trace).
The torch route is the restatement the tests pin, imported from ``tests/tsception_ref.py`` on purpose: the model the
HIP path is compared with for speed is the one it is compared with for values."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import isd_amd
from isd_amd import _lib
from bench_csp import shader_clock_mhz, timed
from tsception_ref import TSception as RefTSception

PEAK_TFLOPS = 157.3


def bench_shape(B, C, T, fs, passes, warmup, hip_only):
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    x = torch.randn(B, C, T, device=dev)
    y = torch.randint(0, 5, (B,), device=dev)
    ref = RefTSception(5, (1, C, T), fs, 15, 15, 32, 0.5).to(dev)
    m = isd_amd.nn.TSception(5, (1, C, T), fs, 15, 15, 32, 0.5)
    m.load_state_dict(ref.state_dict())
    m = m.to(dev)
    tr = isd_amd.Trainer(m, lr=5e-4, weight_decay=1e-2)
    opt = torch.optim.AdamW(ref.parameters(), lr=5e-4, weight_decay=1e-2)
    x4 = x[:, None]

    def torch_step(autocast):
        ref.train()
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            loss = torch.nn.functional.cross_entropy(ref(x4), y)
        loss.backward()
        opt.step()

    def torch_eval(autocast):
        ref.eval()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            ref(x4)

    plan = m._plan_for(T)
    probe = _lib.lib().isd_tsception_temporal_probe

    def temporal(backward):
        ws = tr.path._ws["ts"]      # the path's workspace: a training step has run on it (an eval forward since then
        #                             has rewritten the pooled map and BN_t's coefficients, which does not change the timing)
        _lib.check(probe(plan._h, x.data_ptr(), m.flat_params().data_ptr(), ws.data_ptr(), B, backward, _lib.stream()))

    fns = {"hip_step": lambda: tr.step(x, y), "hip_eval": lambda: tr.path.forward(x)}
    if not hip_only:
        fns.update({"torch_step": lambda: torch_step(False), "torch_eval": lambda: torch_eval(False),
                    "temporal_fwd": lambda: temporal(0), "temporal_bwd": lambda: temporal(1),
                    "torch_step_bf16": lambda: torch_step(True), "torch_eval_bf16": lambda: torch_eval(True)})
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    clk = None
    for p in range(passes):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
        if p == passes - 1:
            tr.step(x, y)
            clk = shader_clock_mhz()                               # probed while that step is still queued
    torch.cuda.synchronize()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    line = {"shape": [B, C, T], "fs": fs, "taps": list(m.taps), "passes": passes, "shader_clock_mhz": clk}
    for k, v in med.items():
        line[f"{k}_ms"] = round(v, 4)
    line["hip_step_trials_per_s"] = round(B / (med["hip_step"] * 1e-3))
    if not hip_only:
        flops = 2.0 * B * C * 15 * sum((T - k + 1) * k for k in m.taps)
        line.update(
            torch_step_trials_per_s=round(B / (med["torch_step"] * 1e-3)),
            torch_over_hip_step=round(med["torch_step"] / med["hip_step"], 2),
            torch_over_hip_eval=round(med["torch_eval"] / med["hip_eval"], 2),
            torch_bf16_over_hip_step=round(med["torch_step_bf16"] / med["hip_step"], 2),
            temporal_fwd_tflops=round(flops / (med["temporal_fwd"] * 1e-3) / 1e12, 2),
            temporal_fwd_fraction_of_fp32_peak=round(flops / (med["temporal_fwd"] * 1e-3) / 1e12 / PEAK_TFLOPS, 3),
            temporal_bwd_tflops=round(2 * flops / (med["temporal_bwd"] * 1e-3) / 1e12, 2),
            temporal_bwd_fraction_of_fp32_peak=round(2 * flops / (med["temporal_bwd"] * 1e-3) / 1e12 / PEAK_TFLOPS, 3),
            hip_step_ms_all=[round(v, 4) for v in ms["hip_step"]],
            torch_step_ms_all=[round(v, 4) for v in ms["torch_step"]])
    print(json.dumps(line), flush=True)
    del ref, opt, tr, m
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--shapes", default="64x64x800@250,350x64x800@250")
    a = ap.parse_args()
    for spec in a.shapes.split(","):
        dims, fs = spec.split("@")
        B, C, T = (int(v) for v in dims.split("x"))
        if B > isd_amd.nn.TSception.MAX_BATCH:
            ap.error(f"{spec}: at most {isd_amd.nn.TSception.MAX_BATCH} trials per pass (DESIGN.md 3.10)")
        bench_shape(B, C, T, int(fs), a.passes, a.warmup, a.hip_only)
    return 0


if __name__ == "__main__":
    sys.exit(main())
