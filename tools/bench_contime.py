"""Time-resolved connectivity (csrc/contime.hip): where the pair kernel stands against the same arithmetic in torch
ops and against the rate at which the complex map it reads can be copied at all, and what share of
``spectral_connectivity_time`` is the transform and what share the pair kernel.

Shapes: the notebook's [350, 64, 795] with 19 frequencies 4-40 Hz and [4096, 64, 512] with 8 frequencies 8-36 Hz, at
250 Hz, float32 and float64; methods 'coh' alone, 'wpli' alone and all eight.  The complex map is produced and consumed
in the trial chunks of the call (CONTIME_CHUNK_BYTES).  Per (shape, dtype, methods) one JSON line:
  call_ms               event-timed median of spectral_connectivity_time on the real data (checks, transform and pair
                        kernel per chunk, concatenation);
  transform_ms          the chunks' TfrPlan calls alone, into one reused buffer;
  pair_ms               the chunks' contime_launch calls alone on that buffer (the last chunk's map: the kernel's time
                        does not depend on the values);
  transform_share, pair_share   those two over call_ms;
  torch_ms, torch_over_hip      the same measures in torch ops on the same chunks, looped over (trial, frequency) blocks
                        so that its [block, C, C, T] intermediates stay under 1 GiB, against pair_ms (< 1: the kernel
                        is slower); timed ``--torch-passes`` times only, it is slow;
  z_copy_ms, pair_over_z_copy   the time of a float4 copy (read + write) of the whole map at the rate of a 1 GiB copy
                        timed in this run, and pair_ms over it: the kernel reads the map once per pair of channel
                        tiles, (tiles + 1) / 2 times in all, and writes next to nothing;
  max_diff_to_torch     largest |kernel - torch ops| over the off-diagonal entries of the first chunk.
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
from isd_amd import tfr as itfr
from bench_csp import shader_clock_mhz, timed

ALL = list(icon.CONTIME_METHODS)
S_BYTES = 256 << 20                  # bound on the torch route's s = w_i conj(w_j) block; with u, |s| and one temporary
#                                      of its size alive the intermediates stay under 1 GiB


def torch_contime(z, names, t0, t1):
    """The measures of ``names`` from z [c, C, F, T] in torch ops -> {name: [c, F, C, C]}."""
    c, C, F, T = z.shape
    w = z[..., t0:t1].permute(0, 2, 1, 3).reshape(c * F, C, t1 - t0)
    per = C * C * (t1 - t0) * z.element_size()
    step = max(1, S_BYTES // per)
    out = {m: [] for m in names}
    for b in range(0, c * F, step):
        wb = w[b:b + step]
        s = wb[:, :, None, :] * wb[:, None, :, :].conj()                     # [block, C, C, T]
        if "coh" in names or "imcoh" in names:
            p = (wb.real ** 2 + wb.imag ** 2).mean(-1)
            den = torch.sqrt(p[:, :, None] * p[:, None, :])
            sm = s.mean(-1)
            if "coh" in names:
                out["coh"].append(sm.abs() / den)
            if "imcoh" in names:
                out["imcoh"].append(sm.imag / den)
        if "plv" in names or "ciplv" in names:
            mag = s.abs()
            e = torch.where(mag > 0, s / mag, torch.zeros_like(s)).mean(-1)
            del mag
            if "plv" in names:
                out["plv"].append(e.abs())
            if "ciplv" in names:
                out["ciplv"].append(e.imag.abs() / torch.sqrt((1 - e.real.abs()) * (1 + e.real.abs())))
        im = s.imag
        if "pli" in names:
            out["pli"].append(torch.sign(im).mean(-1).abs())
        if "dpli" in names:
            out["dpli"].append((0.5 * (torch.sign(im) + 1)).mean(-1))
        if "wpli" in names:
            out["wpli"].append(im.mean(-1).abs() / im.abs().mean(-1))
        if "wpli2_debiased" in names:
            sq = (im * im).sum(-1)
            out["wpli2_debiased"].append((im.sum(-1) ** 2 - sq) / (im.abs().sum(-1) ** 2 - sq))
    return {m: torch.cat(v).reshape(c, F, C, C) for m, v in out.items()}


def bench_shape(shape, freqs, dtype, names, passes, torch_passes, warmup, copy_rate):
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    x = torch.randn(*shape, device=dev, dtype=dtype)
    n, C, T = shape
    F = len(freqs)
    sfreq, freqs, n_cycles = itfr._freqs_cycles(250.0, freqs, 7.0)
    n_taps, taps = itfr._cached_morlet(sfreq, freqs.tobytes(), n_cycles.tobytes(), True)
    plan = itfr._cached_plan(n_taps, taps, 1, dev.index)
    cdtype = torch.complex128 if dtype == torch.float64 else torch.complex64
    per_trial = C * F * T * 2 * x.element_size()
    step = max(1, min(n, icon.CONTIME_CHUNK_BYTES // per_trial))
    chunks = [min(step, n - s) for s in range(0, n, step)]
    zbuf = torch.empty((step, C, F, T), dtype=cdtype, device=dev)
    mask = icon.contime_mask(names)

    def transform():
        for s, c in zip(range(0, n, step), chunks):
            plan(x[s:s + c], "complex", out=zbuf[:c])

    def pair():
        for c in chunks:
            icon.contime_launch(zbuf[:c], mask, 0, T)

    def torch_route():
        for c in chunks:
            torch_contime(zbuf[:c], names, 0, T)

    fns = {"call": lambda: icon.spectral_connectivity_time(x, freqs, method=names, sfreq=250.0),
           "transform": transform, "pair": pair}
    transform()                                                    # zbuf holds the last chunk's map from here on
    c0 = chunks[-1]
    got = icon.contime_launch(zbuf[:c0], mask, 0, T)
    ref = torch_contime(zbuf[:c0], names, 0, T)
    off = ~torch.eye(C, dtype=torch.bool, device=dev)
    order = sorted(names, key=ALL.index)
    agree = max(float(torch.nan_to_num(got[i] - ref[m])[..., off].abs().max()) for i, m in enumerate(order))
    del got, ref
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
            pair()
            clk = shader_clock_mhz()                               # probed while that launch is still queued
    ms["torch"] = [timed(torch_route) for _ in range(torch_passes)]
    med = {k: float(np.median(v)) for k, v in ms.items()}
    z_bytes = n * per_trial
    z_copy_ms = 2 * z_bytes / copy_rate * 1e3
    line = {"shape": list(shape), "freqs": F, "dtype": str(dtype).replace("torch.", ""),
            "methods": names[0] if len(names) == 1 else "all8", "chunks": len(chunks), "passes": passes,
            "torch_passes": torch_passes, "shader_clock_mhz": clk, "max_diff_to_torch": float(f"{agree:.2e}"),
            "z_GB": round(z_bytes / 1e9, 2),
            "intermediate_if_unlooped_GB": round(step * F * C * C * T * 2 * x.element_size() / 1e9, 1)}
    for k, v in med.items():
        line[f"{k}_ms"] = round(v, 3)
    line.update(transform_share=round(med["transform"] / med["call"], 3),
                pair_share=round(med["pair"] / med["call"], 3),
                torch_over_hip=round(med["torch"] / med["pair"], 2),
                copy_GBps_read_plus_write=round(copy_rate / 1e9, 1), z_copy_ms=round(z_copy_ms, 3),
                pair_over_z_copy=round(med["pair"] / z_copy_ms, 2),
                pair_ms_all=[round(v, 3) for v in ms["pair"]])
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--torch-passes", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()      # 1 GiB
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    copy_ms = float(np.median([timed(lambda: dst.copy_(src)) for _ in range(9)]))
    copy_rate = 2 * src.numel() * 4 / (copy_ms * 1e-3)             # a copy reads and writes the bytes
    del src, dst
    for shape, freqs in (((350, 64, 795), np.arange(4.0, 41.0, 2.0)), ((4096, 64, 512), np.arange(8.0, 37.0, 4.0))):
        for dtype in (torch.float32, torch.float64):
            for names in (["coh"], ["wpli"], ALL):
                bench_shape(shape, freqs, dtype, names, a.passes, a.torch_passes, a.warmup, copy_rate)
                torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
