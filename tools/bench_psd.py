"""Welch PSD kernel (csrc/psd.hip): where it stands against a copy of its input and against the same estimate in torch
ops.

Shapes: the notebook's [350, 64, 795] float64 and float32 at n_fft 256, full band and 1-45 Hz; [4096, 64, 512] float32
at n_fft 256; [256, 128, 4096] float32 at 1024 Hz, n_fft 2048, n_overlap 1024, at 0.5-100 Hz and at full band.  Per
shape one JSON line:
  psd_hip_ms            event-timed median of isd_amd.psd_array_welch (mean over segments; includes the segment-mean
                        pre-pass and the workspace allocation from torch's caching allocator);
  psd_plan_ms           the same launches through the cached plan alone, without the argument checks of the
                        public function (the gap to psd_hip_ms is host time the GPU waits for);
  psd_hip_tflops        on 4 K n_per_seg S rows;
  psd_hip_fraction_of_copy_rate   input bytes / time over the rate of a float4 copy of the same bytes (read + write)
                        timed in this run;
  psd_torch_over_hip    against  x.unfold(-1, n_per_seg, step) -> subtract mean -> * window -> torch.fft.rfft(n=n_fft)
                        -> abs() ** 2 -> mean -> slice  (< 1: the kernel is slower than the torch route).
The kernel and its torch counterpart alternate inside one process after a warm-up, and the shader clock is probed
while the last pass is still queued.  Nothing is asserted."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from isd_amd import psd as ipsd
from bench_csp import shader_clock_mhz, timed


def bench_shape(shape, dtype, sfreq, n_fft, n_overlap, fmin, fmax, passes, warmup):
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    x = torch.randn(*shape, device=dev, dtype=dtype)
    T = shape[-1]
    d = ipsd.welch_design(sfreq, T, fmin, fmax, n_fft, n_overlap)
    K, S, rows = d.k_hi - d.k_lo + 1, d.n_segments, x.numel() // T
    w = torch.as_tensor(d.window, device=dev, dtype=dtype)
    scale = torch.as_tensor(d.scale, device=dev, dtype=dtype)
    dst = torch.empty_like(x)

    def torch_route():
        seg = x.unfold(-1, d.n_per_seg, d.step)
        seg = (seg - seg.mean(-1, keepdim=True)) * w
        p = torch.fft.rfft(seg, n=n_fft).abs() ** 2
        return p.mean(-2)[..., d.k_lo:d.k_hi + 1] * scale

    plan = ipsd._cached_plan(d.n_fft, d.n_per_seg, d.n_overlap, d.k_lo, d.k_hi, d.window.tobytes(), float(sfreq), True,
                             dev.index)
    x2 = x.reshape(-1, T)
    fns = {
        "psd_plan": lambda: plan(x2),
        "psd_hip": lambda: ipsd.psd_array_welch(x, sfreq, fmin, fmax, n_fft, n_overlap)[0],
        "psd_torch": torch_route,
        "copy": lambda: dst.copy_(x),
    }
    ref = torch_route()
    agree = float((fns["psd_hip"]() - ref).abs().max() / ref.abs().max())
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
            fns["psd_hip"]()
            clk = shader_clock_mhz()                               # probed while that launch is still queued
    med = {k: float(np.median(v)) for k, v in ms.items()}
    bytes_x = x.numel() * x.element_size()
    copy_rate = 2 * bytes_x / (med["copy"] * 1e-3)                 # a copy reads and writes the bytes
    flop = 4.0 * K * d.n_per_seg * S * rows
    line = {"shape": list(shape), "dtype": str(dtype).replace("torch.", ""), "sfreq": sfreq, "n_fft": n_fft,
            "n_overlap": n_overlap, "band_hz": [fmin, None if np.isinf(fmax) else fmax], "bins": K, "segments": S,
            "passes": passes, "shader_clock_mhz": clk, "max_diff_to_torch_over_max": float(f"{agree:.2e}")}
    for k, v in med.items():
        line[f"{k}_ms"] = round(v, 4)
    line.update(
        psd_hip_tflops=round(flop / (med["psd_hip"] * 1e-3) / 1e12, 2),
        psd_hip_GBps=round(bytes_x / (med["psd_hip"] * 1e-3) / 1e9, 1),
        copy_GBps_read_plus_write=round(copy_rate / 1e9, 1),
        psd_hip_fraction_of_copy_rate=round(bytes_x / (med["psd_hip"] * 1e-3) / copy_rate, 3),
        psd_torch_over_hip=round(med["psd_torch"] / med["psd_hip"], 2),
        psd_hip_ms_all=[round(v, 4) for v in ms["psd_hip"]])
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    inf = float("inf")
    for shape, dtype, sfreq, n_fft, n_overlap, fmin, fmax in (
            ((350, 64, 795), torch.float64, 250.0, 256, 0, 0.0, inf),
            ((350, 64, 795), torch.float64, 250.0, 256, 0, 1.0, 45.0),
            ((350, 64, 795), torch.float32, 250.0, 256, 0, 0.0, inf),
            ((350, 64, 795), torch.float32, 250.0, 256, 0, 1.0, 45.0),
            ((4096, 64, 512), torch.float32, 250.0, 256, 0, 0.0, inf),
            ((256, 128, 4096), torch.float32, 1024.0, 2048, 1024, 0.5, 100.0),
            ((256, 128, 4096), torch.float32, 1024.0, 2048, 1024, 0.0, inf)):
        bench_shape(shape, dtype, sfreq, n_fft, n_overlap, fmin, fmax, a.passes, a.warmup)
    return 0


if __name__ == "__main__":
    sys.exit(main())
