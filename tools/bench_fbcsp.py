"""Filter-bank CSP kernels (csrc/fb.hip: isd_fb_trial_cov, isd_fb_csp_power) against the existing two-kernel route.

Two shapes, BANDS_9, m = 8, fp32 bands: the notebook's [350, 64, 795] at 250 Hz and [4096, 64, 512] at 256 Hz.  Per
shape one JSON line:
  cov     fused entry point against  Filterbank.forward -> trial_covariances on the [n * nb, C, T] view;
  power   fused entry point against  Filterbank.forward -> csp_power per band;
each with the event-timed median of the alternating passes, TFLOP/s counted on 2 nb C^2 T n (cov: the full product; the
kernels compute the upper tiles only) and 2 nb m C T n (power), the ratio existing / fused with the spread of the
passes ((max - min) / median of each route), and the peak extra device memory of both routes.  The routes alternate
inside one process after a warm-up and the shader clock is probed while the last pass is still queued.  A last line
times one full FBCSP fit + transform at the notebook shape (two classes).  Nothing is asserted: a loss reads as a ratio below 1."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import isd_amd
from isd_amd import csp as icsp
from isd_amd import fbcsp
from bench_csp import shader_clock_mhz, timed


def peak_extra(fn):
    """Peak device memory above what is allocated before the call (bytes)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def bench_shape(n, C, T, fs, m, passes, warmup):
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    x = torch.randn(n, C, T, device=dev)
    fb = isd_amd.Filterbank(isd_amd.BANDS_9, fs, 4, "f32")
    nb = fb.n_bands
    w = torch.randn(nb, m, C, device=dev) / C ** 0.5

    def cov_old():
        return icsp.trial_covariances(fb.forward(x).view(n * nb, C, T))

    def power_old():
        y = fb.forward(x)
        return torch.stack([icsp.csp_power(y[:, b], w[b], True) for b in range(nb)], dim=1)

    fns = {"cov_fused": lambda: fbcsp.fb_trial_covariances(x, fb), "cov_existing": cov_old,
           "power_fused": lambda: fbcsp.fb_csp_power(x, fb, w, True), "power_existing": power_old}
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    mem = {k: peak_extra(fn) for k, fn in fns.items()}
    ms = {k: [] for k in fns}
    clk = None
    for p in range(passes):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
        if p == passes - 1:
            fns["cov_fused"]()
            clk = shader_clock_mhz()                               # probed while that launch is still queued
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
    line = {"shape": [n, C, T], "fs": fs, "bands": nb, "m": m, "passes": passes, "shader_clock_mhz": clk}
    for k in fns:
        line[f"{k}_ms"] = round(med[k], 4)
        line[f"{k}_spread"] = round(spread[k], 3)
        line[f"{k}_peak_extra_MB"] = round(mem[k] / 1e6, 1)
    line.update(
        cov_fused_tflops_full_product=round(2.0 * nb * C * C * T * n / (med["cov_fused"] * 1e-3) / 1e12, 2),
        cov_existing_tflops_full_product=round(2.0 * nb * C * C * T * n / (med["cov_existing"] * 1e-3) / 1e12, 2),
        power_fused_tflops=round(2.0 * nb * m * C * T * n / (med["power_fused"] * 1e-3) / 1e12, 3),
        power_existing_tflops=round(2.0 * nb * m * C * T * n / (med["power_existing"] * 1e-3) / 1e12, 3),
        cov_existing_over_fused=round(med["cov_existing"] / med["cov_fused"], 2),
        power_existing_over_fused=round(med["power_existing"] / med["power_fused"], 2),
        cov_fused_ms_all=[round(v, 4) for v in ms["cov_fused"]],
        cov_existing_ms_all=[round(v, 4) for v in ms["cov_existing"]],
        power_fused_ms_all=[round(v, 4) for v in ms["power_fused"]],
        power_existing_ms_all=[round(v, 4) for v in ms["power_existing"]])
    print(json.dumps(line), flush=True)


def bench_estimator(n, C, T, fs, m, K):
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, C, T)).astype(np.float32)
    y = np.arange(n) % K
    xd = torch.as_tensor(X).cuda()
    est = isd_amd.FBCSP(m, sfreq=fs, precision="f32")
    est.fit(xd[:2 * K], y[:2 * K])                                  # plan creation and first launches outside the timing
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    est.fit(xd, y)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    out = est.transform(xd)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(json.dumps({"estimator": "FBCSP", "shape": [n, C, T], "fs": fs, "bands": 9, "m": m, "classes": K,
                      "fit_s": round(t1 - t0, 3), "transform_ms": round((t2 - t1) * 1e3, 3),
                      "features": list(out.shape),
                      "note": "two classes: one eigh per band on the host; with more classes Pham's joint "
                              "diagonaliser (csp.decompose, float64, host) dominates the fit"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--m", type=int, default=8)
    a = ap.parse_args()
    bench_shape(350, 64, 795, 250.0, a.m, a.passes, a.warmup)
    bench_shape(4096, 64, 512, 256.0, a.m, a.passes, a.warmup)
    bench_estimator(350, 64, 795, 250.0, a.m, 2)
    return 0


if __name__ == "__main__":
    sys.exit(main())
