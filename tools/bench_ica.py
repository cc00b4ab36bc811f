"""FastICA kernels (csrc/ica.hip): where they stand against their roofs and against the same arithmetic in torch ops.

Step kernel at the notebook's [350, 64, 795] float64 with m = 20 and m = 64 and at [4096, 64, 512] float32 with
m = 64; apply kernel (M [C, C]) at both shapes.  Per case one JSON line:
  isd_ica_step       event-timed median, GB/s of reading x once and its fraction of a float4 copy of the same bytes
                     (read + write, timed in this run), TFLOP/s counted as 4 m C N (the projection and the product
                     G xᵀ), against  g = tanh(U @ x − b); (g @ x.mT).sum(0); g.sum; (1 − g²).sum  in torch ops;
  isd_spatial_apply  event-timed median, GB/s of reading x and writing out, against  M @ x + bias;
the kernels and their torch counterparts alternate inside one process after a warm-up, and the shader clock is probed
while the last pass is still queued.  A last line times one full ``ICA.fit`` (host loop included, wall clock) on
synthetic notebook-shaped trials and gives its ``n_iter_``.  Nothing is asserted: where a kernel is slower than the
torch route the line says so (``*_torch_over_hip`` < 1)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from isd_amd import ICA, _lib
from isd_amd import ica as iica


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


def torch_step(x, U, b):
    g = torch.tanh(U @ x - b[:, None])
    return (g @ x.mT).sum(0), g.sum((0, 2)), (1.0 - g * g).sum((0, 2))


def bench_shape(n, C, T, dtype, ms_list, passes, warmup):
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    x = torch.randn(n, C, T, device=dev, dtype=dtype)
    dst = torch.empty_like(x)
    M = torch.randn(C, C, device=dev, dtype=dtype) / C ** 0.5
    bias = torch.randn(C, device=dev, dtype=dtype)
    out = torch.empty_like(x)
    fns = {"copy": lambda: dst.copy_(x),
           "apply_hip": lambda: iica.spatial_apply(x, M, bias, out=out),
           "apply_torch": lambda: torch.add(M @ x, bias[:, None])}
    for m in ms_list:
        U = torch.randn(m, C, device=dev, dtype=dtype) / C ** 0.5
        b = torch.randn(m, device=dev, dtype=dtype)
        work = torch.empty(iica.ica_step_work_bytes(n, C, T, m, dtype), dtype=torch.uint8, device=dev)
        fns[f"step_m{m}_hip"] = lambda U=U, b=b, work=work: iica.ica_step(x, U, b, work)
        fns[f"step_m{m}_torch"] = lambda U=U, b=b: torch_step(x, U, b)
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    clk = None
    last = f"step_m{ms_list[-1]}_hip"
    for p in range(passes):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
        if p == passes - 1:
            fns[last]()
            clk = shader_clock_mhz()                               # probed while that launch is still queued
    med = {k: float(np.median(v)) for k, v in ms.items()}
    bytes_x = x.numel() * x.element_size()
    copy_rate = 2 * bytes_x / (med["copy"] * 1e-3)                 # a copy reads and writes the bytes
    head = {"shape": [n, C, T], "dtype": str(dtype).replace("torch.", ""), "passes": passes, "shader_clock_mhz": clk,
            "copy_GBps_read_plus_write": round(copy_rate / 1e9, 1)}
    for m in ms_list:
        hip, ref = med[f"step_m{m}_hip"], med[f"step_m{m}_torch"]
        line = dict(head, kernel="isd_ica_step", m=m, hip_ms=round(hip, 4), torch_ms=round(ref, 4),
                    hip_GBps=round(bytes_x / (hip * 1e-3) / 1e9, 1),
                    hip_fraction_of_copy_rate=round(bytes_x / (hip * 1e-3) / copy_rate, 3),
                    hip_tflops=round(4.0 * m * C * n * T / (hip * 1e-3) / 1e12, 2),
                    torch_over_hip=round(ref / hip, 2), hip_ms_all=[round(v, 4) for v in ms[f"step_m{m}_hip"]])
        print(json.dumps(line), flush=True)
    hip, ref = med["apply_hip"], med["apply_torch"]
    line = dict(head, kernel="isd_spatial_apply", R=C, hip_ms=round(hip, 4), torch_ms=round(ref, 4),
                hip_GBps_read_plus_write=round(2 * bytes_x / (hip * 1e-3) / 1e9, 1),
                hip_fraction_of_copy_rate=round(2 * bytes_x / (hip * 1e-3) / copy_rate, 3),
                hip_tflops=round(2.0 * C * C * n * T / (hip * 1e-3) / 1e12, 2),
                torch_over_hip=round(ref / hip, 2), hip_ms_all=[round(v, 4) for v in ms["apply_hip"]])
    print(json.dumps(line), flush=True)


def bench_fit(n, C, T, m):
    rng = np.random.default_rng(0)
    S = rng.laplace(size=(n, m, T))
    A = rng.standard_normal((C, m))
    x = np.einsum("cm,nmt->nct", A, S) + 0.05 * rng.standard_normal((n, C, T)) + rng.uniform(-3, 3, size=(1, C, 1))
    xd = torch.as_tensor(x).cuda()
    torch.cuda.synchronize()
    line = {"fit": "ICA", "shape": [n, C, T], "dtype": "float64", "m": m}
    for k in range(2):                                             # the second fit has every kernel loaded
        t0 = time.perf_counter()
        est = ICA(m, random_state=0).fit(xd)
        torch.cuda.synchronize()
        line["fit_ms_first" if k == 0 else "fit_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    line["n_iter"] = int(est.n_iter_)
    line["fit_ms_per_iter"] = round(line["fit_ms"] / est.n_iter_, 3)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    bench_shape(350, 64, 795, torch.float64, [20, 64], a.passes, a.warmup)
    bench_shape(4096, 64, 512, torch.float32, [64], a.passes, a.warmup)
    bench_fit(350, 64, 795, 20)
    return 0


if __name__ == "__main__":
    sys.exit(main())
