"""CSP kernels (csrc/csp.hip): where they stand against their roofs and against the same arithmetic in torch ops.

Two shapes: [4096, 64, 512] float32 and the notebook's [350, 64, 795] float64, m = 8 filters.  Per shape one JSON line:
  isd_trial_cov      event-timed median, TFLOP/s counted on the full C x C product (the kernel computes the upper
                     tiles only), GB/s of reading x once, against  X @ X.mT / T;
  isd_csp_power      event-timed median, GB/s of reading x once and its fraction of a float4 copy of the same bytes
                     (read + write, timed in this run), against  ((W @ X) ** 2).mean(-1).log();
  isd_cov_group_mean event-timed median (two classes);
the kernels and their torch counterparts alternate inside one process after a warm-up, and the shader clock is probed
while the last pass is still queued.  Nothing is asserted: where a kernel is slower than the torch route the line
says so (``*_torch_over_hip`` < 1)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from isd_amd import _lib
from isd_amd import csp as icsp


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


_clock_stream = None


def shader_clock_mhz(spin_us=300):
    """One-wave probe on a second stream: shader-clock counter against the constant-rate counter over ~spin_us."""
    global _clock_stream
    L = _lib.lib()
    if _clock_stream is None:
        _clock_stream = torch.cuda.Stream()
    with torch.cuda.stream(_clock_stream):
        out = torch.zeros(2, dtype=torch.int64, device="cuda")
    _lib.check(L.isd_shader_clock_probe(out.data_ptr(), int(spin_us), _clock_stream.cuda_stream))
    _clock_stream.synchronize()
    t, r = (int(v) for v in out.tolist())
    return round(t / r * L.isd_wall_clock_khz() / 1000.0, 1) if r > 0 else None


def bench_shape(n, C, T, dtype, m, passes, warmup):
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    x = torch.randn(n, C, T, device=dev, dtype=dtype)
    w = torch.randn(m, C, device=dev, dtype=dtype) / C ** 0.5
    y = np.arange(n) % 2
    idx, offs = np.argsort(y, kind="stable"), np.array([0, (y == 0).sum(), n])
    cov = icsp.trial_covariances(x)
    dst = torch.empty_like(x)
    fns = {
        "cov_hip": lambda: icsp.trial_covariances(x),
        "cov_torch": lambda: (x @ x.mT) / T,
        "power_hip": lambda: icsp.csp_power(x, w, True),
        "power_torch": lambda: ((w @ x) ** 2).mean(-1).log(),
        "copy": lambda: dst.copy_(x),
        "group_mean_hip": lambda: icsp.cov_group_mean(cov, idx, offs, False),
    }
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
            fns["power_hip"]()
            clk = shader_clock_mhz()                               # probed while that launch is still queued
    med = {k: float(np.median(v)) for k, v in ms.items()}
    bytes_x = x.numel() * x.element_size()
    copy_rate = 2 * bytes_x / (med["copy"] * 1e-3)                 # a copy reads and writes the bytes
    line = {"shape": [n, C, T], "dtype": str(dtype).replace("torch.", ""), "m": m, "passes": passes,
            "shader_clock_mhz": clk}
    for k, v in med.items():
        line[f"{k}_ms"] = round(v, 4)
    line.update(
        cov_hip_tflops_full_product=round(2.0 * n * C * C * T / (med["cov_hip"] * 1e-3) / 1e12, 2),
        cov_hip_GBps=round(bytes_x / (med["cov_hip"] * 1e-3) / 1e9, 1),
        cov_torch_over_hip=round(med["cov_torch"] / med["cov_hip"], 2),
        power_hip_GBps=round(bytes_x / (med["power_hip"] * 1e-3) / 1e9, 1),
        copy_GBps_read_plus_write=round(copy_rate / 1e9, 1),
        power_hip_fraction_of_copy_rate=round(bytes_x / (med["power_hip"] * 1e-3) / copy_rate, 3),
        power_torch_over_hip=round(med["power_torch"] / med["power_hip"], 2),
        cov_hip_ms_all=[round(v, 4) for v in ms["cov_hip"]], power_hip_ms_all=[round(v, 4) for v in ms["power_hip"]])
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--m", type=int, default=8)
    a = ap.parse_args()
    bench_shape(4096, 64, 512, torch.float32, a.m, a.passes, a.warmup)
    bench_shape(350, 64, 795, torch.float64, a.m, a.passes, a.warmup)
    return 0


if __name__ == "__main__":
    sys.exit(main())
