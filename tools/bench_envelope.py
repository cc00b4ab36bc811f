"""Envelope correlation kernels (csrc/envcorr.hip): where they stand against the same arithmetic in torch ops and
against the rate at which the vector units could issue the instructions the pair kernel needs.

Shapes: the notebook's [350, 64, 795] float32 and float64, [4096, 64, 512] float32, [256, 128, 4096] float32; each with
``log`` off and on.  Per (shape, log) one JSON line:
  hilbert_ms            event-timed median of analytic.hilbert_device alone (torch.fft on the device);
  envcorr_ms            isd_amd.connectivity.envcorr_launch on the analytic signal: the row prepass and the pair kernel
                        with the workspace and output allocations from torch's caching allocator;
  rows_ms, pair_ms      device time of the two kernels of one call as torch.profiler reports them (null if the profiler
                        gives no kernel records);
  call_ms               envelope_correlation on the real data: checks, hilbert, both kernels;
  torch_ms, torch_over_hip   the definition in torch ops on the analytic signal, looped over the channel j that the
                        others are orthogonalised against so that its [n, C, T] intermediates stay under 1 GiB, against
                        envcorr_ms (< 1: the kernels are slower);
  pair_valu_floor_ms, pair_fraction_of_valu_peak   log off only: the (trial, tile pair, 256 pairs, sample) slots the
                        pair kernel computes -- diagonal tiles and the padding of the last tile included -- times the
                        vector work of one slot in the float32 kernel: 7 fp32 instructions (product, two fma and an add
                        of the compensated cross product, its modulus, two fma against the pivots) and 10 fp64 ones (3
                        conversions, 6 accumulations, a quarter of ec_j's conversion rounded up), an fp64 instruction
                        counted as two because the part's fp64 vector peak is half its fp32 one (78.6 against 157.3
                        TFLOP/s): 27 issue units, over 256 CUs x 4 SIMDs x 32 lanes a clock at the shader clock probed
                        in this run.  The float64 kernel is held to the same count (its 7 are fp64 too, so its own floor
                        is higher and the fraction understated).  With log on the two logf of a slot are library code
                        whose instructions are not counted here: null.
The routes alternate inside one process after a warm-up, and the shader clock is probed while the last pass is still
queued.  Nothing is asserted."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from isd_amd import analytic
from isd_amd import connectivity as icon
from bench_csp import shader_clock_mhz, timed

SLOT_ISSUE_UNITS = 7 + 2 * 10
LANES_PER_CLOCK = 256 * 4 * 32


def kernel_times(fn):
    """{kernel-name fragment: device ms} of one call of fn, or {} if the profiler records no kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for frag in ("envcorr_rows_kernel", "envcorr_pair_kernel"):
                if frag in ev.key:
                    t = getattr(ev, "device_time_total", None)
                    t = getattr(ev, "cuda_time_total", 0.0) if t is None else t
                    out[frag] = out.get(frag, 0.0) + t / 1e3
        return out
    except Exception as e:                                         # a figure is missing, the run goes on
        print(f"# profiler: {type(e).__name__}: {e}", file=sys.stderr)
        return {}


def torch_envcorr(z, log):
    """The pairwise definition in torch ops, one [n, C, T] intermediate at a time."""
    n, C, T = z.shape
    m = z.abs()
    rm = torch.where(m > 0, 1.0 / m, torch.zeros_like(m))
    a, b = z.real, z.imag
    ur, ui = a * rm, -b * rm                                       # u = conj(z) / m
    e = torch.log(m * m) if log else m
    ec = e - e.mean(-1, keepdim=True)
    se = ec.norm(dim=-1)
    se = torch.where(se == 0, torch.ones_like(se), se)
    corr = torch.empty(n, C, C, dtype=m.dtype, device=z.device)
    for j in range(C):
        o = (a * ui[:, j:j + 1] + b * ur[:, j:j + 1]).abs()           # |Im(z u_j)|, real intermediates only
        if log:
            o = torch.log(o * o)
        oc = o - o.mean(-1, keepdim=True)
        so = oc.norm(dim=-1)
        so = torch.where(so == 0, torch.ones_like(so), so)
        corr[:, :, j] = (oc * ec[:, j:j + 1]).sum(-1) / (se[:, j:j + 1] * so)
    torch.diagonal(corr, dim1=-2, dim2=-1).zero_()
    a = corr.abs()
    return (a + a.transpose(-1, -2)) / 2


def bench_shape(shape, dtype, log, passes, warmup):
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    x = torch.randn(*shape, device=dev, dtype=dtype)
    n, C, T = shape
    z = analytic.hilbert_device(x, T).contiguous()
    flags = icon.ENV_ABSOLUTE | (icon.ENV_LOG if log else 0)
    fns = {
        "hilbert": lambda: analytic.hilbert_device(x, T),
        "envcorr": lambda: icon.envcorr_launch(z, flags),
        "call": lambda: icon.envelope_correlation(x, log=log),
        "torch": lambda: torch_envcorr(z, log),
    }
    ref = fns["torch"]()
    got = fns["envcorr"]()
    agree = float(torch.nan_to_num(got - ref).abs().max())
    del ref, got
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
            fns["envcorr"]()
            clk = shader_clock_mhz()                               # probed while that launch is still queued
    med = {k: float(np.median(v)) for k, v in ms.items()}
    kt = kernel_times(fns["envcorr"])
    pair = kt.get("envcorr_pair_kernel")
    nct = (C + 15) // 16
    slots = n * (nct * (nct + 1) // 2) * 256 * T
    floor = None if (log or not clk) else slots * SLOT_ISSUE_UNITS / (LANES_PER_CLOCK * clk * 1e6) * 1e3
    r4 = lambda v: None if v is None else round(v, 4)              # noqa: E731
    line = {"shape": list(shape), "dtype": str(dtype).replace("torch.", ""), "log": log, "passes": passes,
            "shader_clock_mhz": clk, "max_diff_to_torch": float(f"{agree:.2e}"),
            "intermediate_if_unlooped_GB": round(n * C * C * T * x.element_size() / 1e9, 2)}
    for k, v in med.items():
        line[f"{k}_ms"] = round(v, 4)
    line.update(rows_ms=r4(kt.get("envcorr_rows_kernel")), pair_ms=r4(pair), pair_slots=slots,
                pair_valu_floor_ms=r4(floor),
                pair_fraction_of_valu_peak=None if not (pair and floor) else round(floor / pair, 3),
                torch_over_hip=round(med["torch"] / med["envcorr"], 2),
                envcorr_ms_all=[round(v, 4) for v in ms["envcorr"]])
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    for shape, dtype in (((350, 64, 795), torch.float32), ((350, 64, 795), torch.float64),
                         ((4096, 64, 512), torch.float32), ((256, 128, 4096), torch.float32)):
        for log in (False, True):
            bench_shape(shape, dtype, log, a.passes, a.warmup)
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
