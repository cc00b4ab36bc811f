"""Morlet time-frequency kernel (csrc/tfr.hip): where it stands against the same result in torch ops.

Shapes: the notebook's [350, 64, 795] float64 and float32 at 250 Hz, 4 .. 40 Hz step 1, n_cycles 7 and freqs / 2;
[4096, 64, 512] float32 at 256 Hz, 8 .. 40 Hz step 2, freqs / 2; [64, 128, 4096] float32 at 1024 Hz, 25 log-spaced
frequencies 4 .. 100 Hz, 7 cycles.  Per shape 'power' and 'avg_power' at decim 1 and 'power' at decim 4, one JSON line
each:
  tfr_hip_ms            event-timed median of isd_amd.tfr_array_morlet (includes the output allocation from torch's
                        caching allocator and the host checks);
  tfr_hip_tflops        on 4 flop per (useful tap, kept output sample): zeros of the padded taps are not counted;
  padded_over_useful    the taps the kernel multiplies (a group of eight frequencies is padded to its longest) over
                        the useful ones: what the layout spends on zeros.  Skipped samples (decim > 1) are never
                        computed by the kernel; the torch route computes all of them and slices;
  tfr_hip_out_GBps      bytes of the result / time;
  tfr_torch_over_hip    against  fft(rows, n) * fft(wavelets, n) -> ifft -> slice [::decim] -> abs() ** 2 (-> mean
                        over trials), n the next power of two >= T + longest - 1, in chunks of trials that keep the
                        complex map of a chunk near 2 GB (< 1: the kernel is slower than the torch route);
  *_peak_extra_bytes    rise of torch.cuda.max_memory_allocated over one call, the result included.
The kernel and its torch counterpart alternate inside one process after a warm-up, and the shader clock is probed
while the last pass is still queued.  Nothing is asserted."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from isd_amd import tfr as itfr
from bench_csp import shader_clock_mhz, timed

CHUNK_BYTES = 2 << 30


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    del out
    return int(rise)


def bench_shape(shape, dtype, sfreq, freqs, n_cycles, label, passes, warmup):
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    x = torch.randn(*shape, device=dev, dtype=dtype)
    n, C, T = shape
    cdtype = torch.complex128 if dtype == torch.float64 else torch.complex64
    Ws = itfr.morlet(sfreq, freqs, n_cycles, zero_mean=True)
    n_taps = [len(W) for W in Ws]
    Lmax, F = max(n_taps), len(Ws)
    Hmax = (Lmax - 1) // 2
    nfft = 1 << int(np.ceil(np.log2(T + Lmax - 1)))
    bank = np.zeros((F, Lmax), dtype=np.complex128)                # every wavelet centred on Hmax
    for j, W in enumerate(Ws):
        h = (len(W) - 1) // 2
        bank[j, Hmax - h:Hmax + h + 1] = W
    Wf = torch.fft.fft(torch.as_tensor(bank, device=dev).to(cdtype), n=nfft)            # [F, nfft]
    per = max(1, min(n, CHUNK_BYTES // (C * F * nfft * Wf.element_size())))

    def torch_route(decim, average):
        T_out = -(-T // decim)
        if average:
            acc = torch.zeros(C, F, T_out, device=dev, dtype=dtype)
        else:
            out = torch.empty(n, C, F, T_out, device=dev, dtype=dtype)
        for a in range(0, n, per):
            X = torch.fft.fft(x[a:a + per], n=nfft)                # [per, C, nfft]
            z = torch.fft.ifft(X[:, :, None, :] * Wf)[..., Hmax:Hmax + T:decim]
            p = z.abs() ** 2
            if average:
                acc += p.sum(0)
            else:
                out[a:a + per] = p
        return acc / n if average else out

    plan = itfr.TfrPlan(n_taps, np.concatenate(Ws), 1)
    padded_over_useful = plan.padded_taps / plan.useful_taps
    del plan
    for output, decim in (("power", 1), ("avg_power", 1), ("power", 4)):
        average = output == "avg_power"
        fns = {
            "tfr_hip": lambda: itfr.tfr_array_morlet(x, sfreq, freqs, n_cycles, decim=decim, output=output),
            "tfr_torch": lambda: torch_route(decim, average),
        }
        ref = fns["tfr_torch"]()
        got = fns["tfr_hip"]()
        agree = float((got - ref).abs().max() / ref.abs().max())
        del ref, got
        extra = {k: peak_extra(fn) for k, fn in fns.items()}
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
                fns["tfr_hip"]()
                clk = shader_clock_mhz()                           # probed while that launch is still queued
        med = {k: float(np.median(v)) for k, v in ms.items()}
        T_out = -(-T // decim)
        flop = 4.0 * sum(n_taps) * n * C * T_out
        out_bytes = (C if average else n * C) * F * T_out * x.element_size()
        line = {"shape": list(shape), "dtype": str(dtype).replace("torch.", ""), "sfreq": sfreq, "freqs": label,
                "n_freqs": F, "taps_min_max": [min(n_taps), Lmax], "output": output, "decim": decim, "passes": passes,
                "torch_nfft": nfft, "torch_trials_per_chunk": per, "shader_clock_mhz": clk,
                "max_diff_to_torch_over_max": float(f"{agree:.2e}"),
                "padded_over_useful": round(padded_over_useful, 3)}
        for k, v in med.items():
            line[f"{k}_ms"] = round(v, 4)
        line.update(
            tfr_hip_tflops=round(flop / (med["tfr_hip"] * 1e-3) / 1e12, 2),
            tfr_hip_out_GBps=round(out_bytes / (med["tfr_hip"] * 1e-3) / 1e9, 1),
            tfr_torch_over_hip=round(med["tfr_torch"] / med["tfr_hip"], 2),
            tfr_hip_peak_extra_bytes=extra["tfr_hip"], tfr_torch_peak_extra_bytes=extra["tfr_torch"],
            tfr_hip_ms_all=[round(v, 4) for v in ms["tfr_hip"]])
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", type=int, default=None, help="index of the one configuration to run")
    a = ap.parse_args()
    f_nb, f_b = np.arange(4.0, 41.0), np.arange(8.0, 41.0, 2.0)
    f_log = np.geomspace(4.0, 100.0, 25)
    configs = (
        ((350, 64, 795), torch.float64, 250.0, f_nb, 7.0, "4..40 step 1, 7 cycles"),
        ((350, 64, 795), torch.float64, 250.0, f_nb, f_nb / 2.0, "4..40 step 1, freqs/2 cycles"),
        ((350, 64, 795), torch.float32, 250.0, f_nb, 7.0, "4..40 step 1, 7 cycles"),
        ((350, 64, 795), torch.float32, 250.0, f_nb, f_nb / 2.0, "4..40 step 1, freqs/2 cycles"),
        ((4096, 64, 512), torch.float32, 256.0, f_b, f_b / 2.0, "8..40 step 2, freqs/2 cycles"),
        ((64, 128, 4096), torch.float32, 1024.0, f_log, 7.0, "4..100 log-spaced x25, 7 cycles"))
    for i, (shape, dtype, sfreq, freqs, n_cycles, label) in enumerate(configs):
        if a.only is None or a.only == i:
            bench_shape(shape, dtype, sfreq, freqs, n_cycles, label, a.passes, a.warmup)
    return 0


if __name__ == "__main__":
    sys.exit(main())
