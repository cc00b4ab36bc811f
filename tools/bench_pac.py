"""Phase-amplitude coupling kernels (csrc/pac.hip): where they stand against the same arithmetic in torch ops and
against the rates at which the vector units and the LDS could serve the main kernel's inner loop.

Case 1: the notebook's [350, 64, 795], nine 2-Hz phase bands over 2-20 Hz, nine 10-Hz amplitude bands over 30-120 Hz,
S = 0 and S = 200, float32 and float64.  Case 2: [4096, 64, 512] float32, P = 2, A = 4, S = 200.  One JSON line each:
  pac_ms                  event-timed median of isd_amd.pac.pac_launch on ready phases and amplitudes: the three
                          kernels with the workspace and output allocations from torch's caching allocator;
  sort_ms, order_ms, main_ms   device time of the kernels of one call as torch.profiler reports them (null if the
                          profiler gives no kernel records);
  call_ms, plumbing_fraction   phase_amplitude_coupling on the real data (checks, a zero-phase FIR, an FFT pair and an
                          angle or modulus per band, stacking, the kernels), and (call_ms - pac_ms) / call_ms: how much
                          of the whole call is filter + FFT plumbing;
  torch_ms, torch_route, torch_over_hip   the same arithmetic in torch ops: rows in chunks so that the largest
                          intermediate stays under 1 GiB, a loop over the shifts, the bin sums by a one-hot einsum or
                          by scatter_add_ (index_add_ with a per-row index), whichever was faster in one timed pass
                          each, the complex mean by two einsums; against pac_ms (< 1: the kernels are slower).  With
                          S = 200 it is timed once;
  main_valu_floor_ms, main_lds_floor_ms, main_fraction_of_floor   the lane slots the main kernel walks -- rows x A x P
                          x ceil(ceil((1 + S) / 32) / 2) groups of 64 lanes x T samples, idle lanes included -- times
                          the inner loop's vector work as compiled: float32 one address add, one packed fma (re and im)
                          and one add, 3 issue units; float64 one address add, two fma and one add in fp64, an fp64
                          instruction counted as two, 7 units; over 256 CUs x 4 SIMDs x 32 lanes a clock.  The LDS
                          floor is one gathered read per wave and sample at 2 LDS cycles (conflict-free ds_read_b32 /
                          b64) over 256 CUs.  The fraction is max(floors) / main_ms, at the shader clock probed in this
                          run;
  useful_lane_fraction    (1 + S) / (64 x groups): with S = 0 one lane in 64 works.
The routes alternate inside one process after a warm-up, and the shader clock is probed while the last pass is still
queued.  Nothing is asserted."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from isd_amd import pac as ipac
from bench_csp import shader_clock_mhz, timed

LANES_PER_CLOCK = 256 * 4 * 32
CUS = 256
ISSUE_UNITS = {torch.float32: 3, torch.float64: 7}
KERNELS = ("pac_sort_kernel", "pac_order_kernel", "pac_main_kernel")


def kernel_times(fn):
    """{kernel-name fragment: device ms} of one call of fn, or {} if the profiler records no kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for frag in KERNELS:
                if frag in ev.key:
                    t = getattr(ev, "device_time_total", None)
                    t = getattr(ev, "cuda_time_total", 0.0) if t is None else t
                    out[frag] = out.get(frag, 0.0) + t / 1e3
        return out
    except Exception as e:                                         # a figure is missing, the run goes on
        print(f"# profiler: {type(e).__name__}: {e}", file=sys.stderr)
        return {}


def torch_pac(pha, amp, shifts, B, route):
    """The definitions in torch ops: pha [R, P, T], amp [R, A, T] -> [R, A, P, 3, 1 + S] (mvl, mi, hr per shift)."""
    R, P, T = pha.shape
    A = amp.shape[1]
    es = pha.element_size()
    step = max(1, (1 << 30) // (P * T * B * es if route == "onehot" else A * P * T * 8))
    out = torch.empty(R, A, P, 3, len(shifts), dtype=pha.dtype, device=pha.device)
    for r0 in range(0, R, step):
        ph, am = pha[r0:r0 + step], amp[r0:r0 + step]
        b = ((ph.double() + math.pi) * (B / (2.0 * math.pi))).floor().clamp_(0, B - 1).long()
        n_j = torch.zeros(ph.shape[0], P, B, dtype=pha.dtype, device=pha.device).scatter_add_(
            -1, b, torch.ones_like(ph))
        rn = torch.where(n_j > 0, 1.0 / n_j, torch.zeros_like(n_j))[:, None]          # [r, 1, P, B]
        cs, sn = torch.cos(ph), torch.sin(ph)
        if route == "onehot":
            onehot = torch.nn.functional.one_hot(b, B).to(pha.dtype)                   # [r, P, T, B]
        else:
            bi = b[:, None].expand(-1, A, -1, -1)                                      # [r, A, P, T]
        for i, s in enumerate(shifts):
            a_s = torch.roll(am, -int(s), -1)
            re = torch.einsum("rat,rpt->rap", a_s, cs)
            im = torch.einsum("rat,rpt->rap", a_s, sn)
            if route == "onehot":
                sums = torch.einsum("rat,rptb->rapb", a_s, onehot)
            else:
                sums = torch.zeros(ph.shape[0], A, P, B, dtype=pha.dtype, device=pha.device).scatter_add_(
                    -1, bi, a_s[:, :, None, :].expand(-1, -1, P, -1))
            m = sums * rn
            Pj = m / m.sum(-1, keepdim=True)
            out[r0:r0 + step, :, :, 0, i] = torch.sqrt(re * re + im * im) / T
            out[r0:r0 + step, :, :, 1, i] = 1.0 + torch.xlogy(Pj, Pj).sum(-1) / math.log(B)
            mx = m.amax(-1)
            out[r0:r0 + step, :, :, 2, i] = (mx - m.amin(-1)) / mx
    return out


def bench_case(shape, dtype, f_pha, f_amp, S, passes, warmup, sfreq=250.0, B=18):
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    n, C, T = shape
    P, A = len(f_pha), len(f_amp)
    x = torch.randn(*shape, device=dev, dtype=dtype)
    pha = ((torch.rand(n * C, P, T, device=dev, dtype=torch.float64) * 2 - 1) * math.pi).to(dtype)
    amp = (1 + torch.randn(n * C, A, T, device=dev, dtype=dtype)).abs()
    shifts = ipac.draw_shifts(T, S, 0)
    sd = torch.from_numpy(shifts).to(dev)
    fns = {
        "pac": lambda: ipac.pac_launch(pha, amp, sd, B, surrogates_out=S > 0),
        "call": lambda: ipac.phase_amplitude_coupling(x, sfreq, f_pha, f_amp, method=list(ipac.METHODS), n_bins=B,
                                                      shifts=shifts, return_stats=True),
    }
    # the torch route: a subset of the rows decides which bin sum is faster and checks the kernels
    sub = slice(0, min(n * C, 256))
    got = ipac.pac_launch(pha[sub].contiguous(), amp[sub].contiguous(), sd, B, surrogates_out=True)
    got = torch.cat([got[0][..., :1], got[1]], -1)
    route_ms, agree = {}, None
    for route in ("onehot", "scatter"):
        ref = torch_pac(pha[sub], amp[sub], shifts, B, route)            # also the warm-up of this route
        agree = float(torch.nan_to_num(got - ref).abs().max())
        route_ms[route] = timed(lambda: torch_pac(pha[sub], amp[sub], shifts, B, route))
        del ref
    route = min(route_ms, key=route_ms.get)
    del got
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
            fns["pac"]()
            clk = shader_clock_mhz()                               # probed while that launch is still queued
    med = {k: float(np.median(v)) for k, v in ms.items()}
    torch_ms = float(np.median([timed(lambda: torch_pac(pha, amp, shifts, B, route))
                                for _ in range(1 if S else passes)]))
    kt = kernel_times(fns["pac"])
    main = kt.get("pac_main_kernel")
    groups = ((1 + S + 31) // 32 + 1) // 2
    wave_samples = n * C * A * P * groups * T
    valu = lds = None
    if clk:
        valu = wave_samples * 64 * ISSUE_UNITS[dtype] / (LANES_PER_CLOCK * clk * 1e6) * 1e3
        lds = wave_samples * 2 / (CUS * clk * 1e6) * 1e3
    r4 = lambda v: None if v is None else round(v, 4)              # noqa: E731
    line = {"shape": list(shape), "dtype": str(dtype).replace("torch.", ""), "P": P, "A": A, "S": S, "n_bins": B,
            "passes": passes, "shader_clock_mhz": clk, "max_diff_to_torch": float(f"{agree:.2e}"),
            "gather_if_unlooped_GB": round(n * C * A * max(S, 1) * T * x.element_size() / 1e9, 2)}
    for k, v in med.items():
        line[f"{k}_ms"] = round(v, 4)
    line.update(sort_ms=r4(kt.get("pac_sort_kernel")), order_ms=r4(kt.get("pac_order_kernel")), main_ms=r4(main),
                plumbing_fraction=round((med["call"] - med["pac"]) / med["call"], 3),
                torch_ms=round(torch_ms, 3), torch_route=route,
                torch_subset_ms={k: round(v, 3) for k, v in route_ms.items()},
                torch_over_hip=round(torch_ms / med["pac"], 2),
                main_valu_floor_ms=r4(valu), main_lds_floor_ms=r4(lds),
                main_fraction_of_floor=None if not (main and valu) else round(max(valu, lds) / main, 3),
                useful_lane_fraction=round((1 + S) / (64 * groups), 3),
                pac_ms_all=[round(v, 4) for v in ms["pac"]])
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="1,2")
    a = ap.parse_args()
    pha9 = [(2.0 + 2 * i, 4.0 + 2 * i) for i in range(9)]
    amp9 = [(30.0 + 10 * i, 40.0 + 10 * i) for i in range(9)]
    cases = a.cases.split(",")
    if "1" in cases:
        for dtype in (torch.float32, torch.float64):
            for S in (0, 200):
                bench_case((350, 64, 795), dtype, pha9, amp9, S, a.passes, a.warmup)
                torch.cuda.empty_cache()
    if "2" in cases:
        bench_case((4096, 64, 512), torch.float32, [(4.0, 8.0), (8.0, 13.0)],
                   [(30.0, 50.0), (50.0, 70.0), (70.0, 90.0), (90.0, 110.0)], 200, a.passes, a.warmup)
    return 0


if __name__ == "__main__":
    sys.exit(main())
