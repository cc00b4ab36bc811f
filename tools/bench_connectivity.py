"""Cross-spectral density kernels (csrc/csd.hip): where they stand against the same estimate in torch ops and against
the rate at which their output can be written at all.

Shapes: the notebook's [350, 64, 795] float64 and float32 at n_fft 256, n_overlap 128, at 1-45 Hz and at full band;
[4096, 64, 512] float32 at full band; each in both averaging modes.  Per (shape, mode) one JSON line:
  csd_hip_ms            event-timed median of isd_amd.connectivity.csd_array_welch (segment means, spectra, product,
                        the workspace and output allocations from torch's caching allocator);
  spectra_ms, product_ms, mean_ms, reduce_ms
                        device time of the kernels of one call as torch.profiler reports them (null if the profiler
                        gives no kernel records);
  product_fraction_of_copy_rate   output bytes / product_ms over the rate of a float4 copy (read + write) of 1 GiB
                        timed in this run: the product kernel's roofline is writing C^2 K complex values per trial;
  csd_torch_over_hip    against  x.unfold(-1, n_per_seg, step) -> subtract mean -> * window -> torch.fft.rfft(n=n_fft)
                        -> slice -> einsum('...isk,...jsk->...kij') -> scale  (< 1: the kernels are slower);
  csd_unit_ms           the unit-modulus pass alone (csd_launch on the cached plan, timed like csd_hip);
  con_ms, con_elementwise_share   spectral_connectivity(method=['coh', 'plv']) (a density and a unit-modulus pass
                        plus the elementwise torch step) and 1 - (csd_hip_ms + csd_unit_ms) / con_ms, the share of it
                        that is neither pass: the number that says whether a fused measure epilogue is worth
                        building.  csd_hip_ms carries the argument checks of the public function, which
                        spectral_connectivity pays once, so the share is understated by that much.
The routes alternate inside one process after a warm-up, and the shader clock is probed while the last pass is still
queued.  Nothing is asserted."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from isd_amd import connectivity as icon
from isd_amd import psd as ipsd
from bench_csp import shader_clock_mhz, timed


def kernel_times(fn):
    """{kernel-name fragment: device ms} of one call of fn, or {} if the profiler records no kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for frag in ("psd_mean_kernel", "csd_spectra_kernel", "csd_product_kernel", "csd_reduce_kernel"):
                if frag in ev.key:
                    t = getattr(ev, "device_time_total", None)
                    t = getattr(ev, "cuda_time_total", 0.0) if t is None else t
                    out[frag] = out.get(frag, 0.0) + t / 1e3
        return out
    except Exception as e:                                         # a figure is missing, the run goes on
        print(f"# profiler: {type(e).__name__}: {e}", file=sys.stderr)
        return {}


def bench_shape(shape, dtype, sfreq, n_fft, n_overlap, fmin, fmax, average, passes, warmup, copy_rate):
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    x = torch.randn(*shape, device=dev, dtype=dtype)
    n, C, T = shape
    d = ipsd.welch_design(sfreq, T, fmin, fmax, n_fft, n_overlap, window="hann")
    K, S = d.k_hi - d.k_lo + 1, d.n_segments
    w = torch.as_tensor(d.window, device=dev, dtype=dtype)
    scale = torch.as_tensor(d.scale, device=dev, dtype=dtype)[:, None, None]
    over = average == "trials"
    args = dict(sfreq=sfreq, fmin=fmin, fmax=fmax, n_fft=n_fft, n_overlap=n_overlap, average=average)

    def torch_route():
        seg = x.unfold(-1, d.n_per_seg, d.step)
        seg = (seg - seg.mean(-1, keepdim=True)) * w
        X = torch.fft.rfft(seg, n=n_fft)[..., d.k_lo:d.k_hi + 1]
        if over:
            return torch.einsum("nisk,njsk->kij", X, X.conj()) * (scale / (n * S))
        return torch.einsum("nisk,njsk->nkij", X, X.conj()) * (scale / S)

    plan = ipsd._cached_plan(d.n_fft, d.n_per_seg, d.n_overlap, d.k_lo, d.k_hi, d.window.tobytes(), float(sfreq), True,
                             dev.index)
    fns = {
        "csd_hip": lambda: icon.csd_array_welch(x, **args)[0],
        "csd_torch": torch_route,
        "csd_unit": lambda: icon.csd_launch(plan, x, over, unit_modulus=True),
        "con": lambda: icon.spectral_connectivity(x, method=["coh", "plv"], **args)[0],
    }
    ref = torch_route()
    agree = float((fns["csd_hip"]() - ref).abs().max() / ref.abs().max())
    del ref
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
            fns["csd_hip"]()
            clk = shader_clock_mhz()                               # probed while that launch is still queued
    med = {k: float(np.median(v)) for k, v in ms.items()}
    kt = kernel_times(fns["csd_hip"])
    out_bytes = (1 if over else n) * K * C * C * 2 * x.element_size()
    prod = kt.get("csd_product_kernel")
    line = {"shape": list(shape), "dtype": str(dtype).replace("torch.", ""), "average": average, "n_fft": n_fft,
            "n_overlap": n_overlap, "band_hz": [fmin, None if np.isinf(fmax) else fmax], "bins": K, "segments": S,
            "passes": passes, "shader_clock_mhz": clk, "max_diff_to_torch_over_max": float(f"{agree:.2e}"),
            "out_MB": round(out_bytes / 1e6, 1)}
    for k, v in med.items():
        line[f"{k}_ms"] = round(v, 4)
    r4 = lambda v: None if v is None else round(v, 4)              # noqa: E731
    line.update(
        mean_ms=r4(kt.get("psd_mean_kernel")), spectra_ms=r4(kt.get("csd_spectra_kernel")), product_ms=r4(prod),
        reduce_ms=r4(kt.get("csd_reduce_kernel")),
        product_out_GBps=None if not prod else round(out_bytes / (prod * 1e-3) / 1e9, 1),
        copy_GBps_read_plus_write=round(copy_rate / 1e9, 1),
        product_fraction_of_copy_rate=None if not prod else round(out_bytes / (prod * 1e-3) / copy_rate, 3),
        csd_torch_over_hip=round(med["csd_torch"] / med["csd_hip"], 2),
        con_elementwise_share=round(max(0.0, 1.0 - (med["csd_hip"] + med["csd_unit"]) / med["con"]), 3),
        csd_hip_ms_all=[round(v, 4) for v in ms["csd_hip"]])
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    inf = float("inf")
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()      # 1 GiB
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    copy_ms = float(np.median([timed(lambda: dst.copy_(src)) for _ in range(9)]))
    copy_rate = 2 * src.numel() * 4 / (copy_ms * 1e-3)             # a copy reads and writes the bytes
    del src, dst
    for shape, dtype, fmin, fmax in (
            ((350, 64, 795), torch.float64, 1.0, 45.0),
            ((350, 64, 795), torch.float64, 0.0, inf),
            ((350, 64, 795), torch.float32, 1.0, 45.0),
            ((350, 64, 795), torch.float32, 0.0, inf),
            ((4096, 64, 512), torch.float32, 0.0, inf)):
        for average in ("segments", "trials"):
            bench_shape(shape, dtype, 250.0, 256, 128, fmin, fmax, average, a.passes, a.warmup, copy_rate)
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
