"""Polyphase resampling kernel (csrc/resample.hip): where it stands against a copy of its bytes and against the same
arithmetic in torch ops.

Shapes: [2048, 128, 4096] float32 at 1/4 (1024 -> 256 Hz) and 125/512 (1024 -> 250 Hz); [4096, 64, 512] float32 at 1/2
and 2/1; the notebook's [350, 64, 795] float64 at 1/2 and 128/125 (250 -> 256 Hz).  Per shape one JSON line:
  rs_hip_ms             event-timed median of isd_amd.resample_poly (padtype 'constant'; includes the output's
                        allocation from torch's caching allocator);
  rs_plan_ms            the same launch through the cached plan alone, without the argument checks of the public
                        function (the gap to rs_hip_ms is host time the GPU waits for);
  rs_hip_tflops         on 2 K 16 flop per block of 16 outputs and row: what the matrix cores are issued, zeros included;
  rs_hip_fraction_of_copy_rate   (bytes of x + bytes of y) / time over the rate of a float4 copy (read + write) timed in
                        this run: the roofline of a kernel that reads x once and writes y once;
  rs_torch_over_hip     against torchaudio's algorithm in torch ops: F.pad of the row, then
                        F.conv1d(x[:, None], phases[up, 1, W], stride=down) and the phase outputs interleaved
                        (< 1: the kernel is slower than the torch route).
  *_max_diff_to_scipy_over_max   both routes on eight rows spread over the batch against scipy.signal.resample_poly
                        in float64 on the host; max_diff_to_torch_over_max the two routes against each other, all rows.
The kernel and its comparators alternate inside one process after a warm-up, and the shader clock is probed while the
last pass is still queued.  Nothing is asserted."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
from scipy import signal

from isd_amd import resampling as rs
from bench_csp import shader_clock_mhz, timed


def phase_filters(d):
    """The design as ``up`` filters over s = s_min .. s_max: w[i][s − s_min] = h[half_len + i down − s up], so that
    y[up t + i] = Σ_s w[i][s − s_min] x[t down + s]."""
    L = d.taps.size
    i = np.arange(d.up)
    s_min = int(np.min(-((L - 1 - d.half_len - i * d.down) // d.up)))
    s_max = int(np.max((d.half_len + i * d.down) // d.up))
    idx = d.half_len + i[:, None] * d.down - np.arange(s_min, s_max + 1)[None, :] * d.up
    return np.where((idx >= 0) & (idx < L), d.taps[np.clip(idx, 0, L - 1)], 0.0), s_min


def bench_shape(shape, dtype, up, down, passes, warmup, with_torch=True):
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    x = torch.randn(*shape, device=dev, dtype=dtype)
    T = shape[-1]
    d = rs.resample_design(up, down)
    n_out, rows = rs.out_len(T, up, down), x.numel() // T
    w_np, s_min = phase_filters(d)
    w = torch.as_tensor(w_np, device=dev, dtype=dtype)[:, None, :]
    W, n_t = w.shape[-1], -(-n_out // d.up)
    left = max(-s_min, 0)
    right = max((n_t - 1) * d.down + max(s_min, 0) + W - (left + T), 0)
    x2 = x.reshape(rows, T)
    dst = torch.empty_like(x)

    def torch_route():
        xp = F.pad(x2, (left, right))[:, None, max(s_min, 0):]
        y = F.conv1d(xp, w, stride=d.down)[..., :n_t]              # [rows, up, n_t]
        return y.transpose(1, 2).reshape(rows, n_t * d.up)[:, :n_out]

    plan = rs._cached_plan(d.up, d.down, ("kaiser", 5.0), None, dev.index)
    fns = {
        "rs_plan": lambda: plan(x2),
        "rs_hip": lambda: rs.resample_poly(x, up, down),
        "rs_torch": torch_route,
        "copy": lambda: dst.copy_(x),
    }
    # eight rows spread over the batch against scipy in float64 on the host, for both routes
    pick = torch.linspace(0, rows - 1, 8, device=dev).long()
    ref = torch.as_tensor(signal.resample_poly(x2[pick].double().cpu().numpy(), up, down, axis=-1), device=dev)
    to_scipy = lambda y: float(f"{float((y[pick].double() - ref).abs().max() / ref.abs().max()):.2e}")  # noqa: E731
    agree = {"rs_hip_max_diff_to_scipy_over_max": to_scipy(fns["rs_plan"]())}
    if with_torch:
        agree["rs_torch_max_diff_to_scipy_over_max"] = to_scipy(torch_route())
        agree["max_diff_to_torch_over_max"] = float(f"{float((fns['rs_plan']() - torch_route()).abs().max() / ref.abs().max()):.2e}")
    else:
        del fns["rs_torch"]
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
            fns["rs_hip"]()
            clk = shader_clock_mhz()                               # probed while that launch is still queued
    med = {k: float(np.median(v)) for k, v in ms.items()}
    es = x.element_size()
    bytes_x, bytes_y = x.numel() * es, rows * n_out * es
    copy_rate = 2 * bytes_x / (med["copy"] * 1e-3)                 # a copy reads and writes the bytes
    n_phase, K = rs.phase_tables_shape(d)
    flop = 2.0 * K * 16 * 16 * (-(-n_out // 16)) * (-(-rows // 16))
    line = {"shape": list(shape), "dtype": str(dtype).replace("torch.", ""), "up": d.up, "down": d.down, "n_out": n_out,
            "taps": int(d.taps.size), "phase_tables": n_phase, "window_samples_per_block": K, "passes": passes, "shader_clock_mhz": clk, **agree}
    for k, v in med.items():
        line[f"{k}_ms"] = round(v, 4)
    line.update(
        rs_hip_tflops=round(flop / (med["rs_hip"] * 1e-3) / 1e12, 2),
        rs_hip_GBps=round((bytes_x + bytes_y) / (med["rs_hip"] * 1e-3) / 1e9, 1),
        copy_GBps_read_plus_write=round(copy_rate / 1e9, 1),
        rs_hip_fraction_of_copy_rate=round((bytes_x + bytes_y) / (med["rs_hip"] * 1e-3) / copy_rate, 3),
        rs_torch_over_hip=round(med["rs_torch"] / med["rs_hip"], 2) if with_torch else None,
        rs_hip_ms_all=[round(v, 4) for v in ms["rs_hip"]])
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="leave the torch route out (its first call tunes a convolution)")
    ap.add_argument("--only", type=int, default=None, help="index of the one shape to run")
    a = ap.parse_args()
    cases = (((2048, 128, 4096), torch.float32, 1, 4),
             ((2048, 128, 4096), torch.float32, 125, 512),
             ((4096, 64, 512), torch.float32, 1, 2),
             ((4096, 64, 512), torch.float32, 2, 1),
             ((350, 64, 795), torch.float64, 1, 2),
             ((350, 64, 795), torch.float64, 128, 125))
    for i, (shape, dtype, up, down) in enumerate(cases):
        if a.only is None or a.only == i:
            bench_shape(shape, dtype, up, down, a.passes, a.warmup, not a.no_torch)
    return 0


if __name__ == "__main__":
    sys.exit(main())
