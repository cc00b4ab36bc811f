"""Riemannian kernels (csrc/riemann.hip): where they stand against the same arithmetic in torch ops on the same card.

Four fp64 stacks, [350, 64, 64], [4096, 64, 64], [2048, 128, 128] and [4096, 16, 16]: covariances of synthetic trials
whitened by their arithmetic mean (what the pipeline hands to the eigen kernel).  Per stack one JSON line:
  isd_spd_eigfun(LOG, TANGENT)  event-timed median, mean Jacobi sweeps per matrix (from info) and time per sweep,
                                against  torch.linalg.eigh -> V log(Λ) Vᵀ -> triu with √2;
  isd_spd_congruence            event-timed median, GFLOP/s counted on both full products, against  W @ cov @ W.mT.
Then the notebook's [350, 64, 795] trials: one TangentSpace.fit + transform and one five-class MDM.fit, with the mean
iterations, the time inside the two kernels (event-timed per call, summed) and the rest (host eigh of the class means,
transfers, torch ops).  The kernels and their torch counterparts alternate inside one process after a warm-up, and
the shader clock is probed while the last pass is still queued.  Nothing is asserted: where a kernel is slower than
the torch route the line says so (``*_torch_over_hip`` < 1)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from isd_amd import _lib
from isd_amd import csp as icsp
from isd_amd import riemann as rm


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


def whitened_stack(n, C, seed=0):
    """[n, C, C] fp64 on the card: covariances of [n, C, 4 C] mixed noise, whitened by their arithmetic mean."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    mix = torch.randn(C, C, device="cuda", dtype=torch.float64, generator=g) / C ** 0.5 \
        + torch.eye(C, device="cuda", dtype=torch.float64)
    cov = torch.empty(n, C, C, device="cuda", dtype=torch.float64)
    for s in range(0, n, 512):
        x = mix @ torch.randn(min(512, n - s), C, 4 * C, device="cuda", dtype=torch.float64, generator=g)
        cov[s:s + 512] = icsp.trial_covariances(x)
    lam, V = torch.linalg.eigh(cov.mean(0))
    W = (V * lam.rsqrt()) @ V.mT
    return cov, W, rm.congruence(cov, W)


def torch_log_tangent(a, iu, coef):
    lam, V = torch.linalg.eigh(a)
    full = (V * lam.log().unsqueeze(-2)) @ V.mT
    return full[:, iu[0], iu[1]] * coef


def bench_stack(n, C, passes, warmup):
    cov, W, a = whitened_stack(n, C)
    iu = torch.triu_indices(C, C, device="cuda")
    coef = torch.full((iu.shape[1],), 2.0 ** 0.5, dtype=torch.float64, device="cuda")
    coef[iu[0] == iu[1]] = 1.0
    Wk = W[None].contiguous()
    fns = {
        "eigfun_hip": lambda: rm._eigfun(a, rm.SPD_LOG, rm.SPD_TANGENT, False),
        "eigfun_torch": lambda: torch_log_tangent(a, iu, coef),
        "congruence_hip": lambda: rm.congruence(cov, Wk),
        "congruence_torch": lambda: W @ cov @ W.mT,
    }
    got, _, info = fns["eigfun_hip"]()
    want = fns["eigfun_torch"]()
    agree = float((got - want).abs().max() / want.abs().max())
    cong = float((fns["congruence_hip"]() - fns["congruence_torch"]()).abs().max() / a.abs().max())
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
            fns["eigfun_hip"]()
            clk = shader_clock_mhz()                               # probed while that launch is still queued
    med = {k: float(np.median(v)) for k, v in ms.items()}
    sweeps = float(info.double().mean())
    line = {"shape": [n, C, C], "dtype": "float64", "passes": passes, "shader_clock_mhz": clk,
            "failed_matrices": int((info <= 0).sum())}
    for k, v in med.items():
        line[f"{k}_ms"] = round(v, 4)
    line.update(
        eigfun_torch_over_hip=round(med["eigfun_torch"] / med["eigfun_hip"], 2),
        eigfun_mean_sweeps=round(sweeps, 2), eigfun_max_sweeps=int(info.max()),
        eigfun_us_per_matrix=round(med["eigfun_hip"] * 1e3 / n, 3),
        eigfun_ms_per_sweep_of_the_batch=round(med["eigfun_hip"] / sweeps, 4),
        eigfun_hip_vs_torch_max_rel=agree,
        congruence_torch_over_hip=round(med["congruence_torch"] / med["congruence_hip"], 2),
        congruence_hip_gflops_full_products=round(4.0 * n * C ** 3 / (med["congruence_hip"] * 1e-3) / 1e9, 1),
        congruence_hip_vs_torch_max_rel=cong,
        eigfun_hip_ms_all=[round(v, 4) for v in ms["eigfun_hip"]],
        congruence_hip_ms_all=[round(v, 4) for v in ms["congruence_hip"]])
    print(json.dumps(line), flush=True)


class KernelClock:
    """Event-times every call of rm.congruence and rm._eigfun while active (adds a synchronise per call)."""

    def __enter__(self):
        self.ms, self.calls = 0.0, 0
        self._saved = (rm.congruence, rm._eigfun)

        def wrap(fn):
            def inner(*a, **k):
                box = []
                self.ms += timed(lambda: box.append(fn(*a, **k)))
                self.calls += 1
                return box[0]
            return inner
        rm.congruence, rm._eigfun = wrap(rm.congruence), wrap(rm._eigfun)
        return self

    def __exit__(self, *exc):
        rm.congruence, rm._eigfun = self._saved


def bench_pipeline(passes, warmup):
    n, C, T, K = 350, 64, 795, 5
    g = torch.Generator(device="cuda").manual_seed(1)
    y = np.arange(n) % K
    mix = torch.randn(K, C, C, device="cuda", dtype=torch.float64, generator=g) * (0.3 / C ** 0.5) \
        + torch.eye(C, device="cuda", dtype=torch.float64)
    x = mix[torch.as_tensor(y).cuda()] @ torch.randn(n, C, T, device="cuda", dtype=torch.float64, generator=g)
    cov = rm.Covariances().transform(x)
    line = {"pipeline": [n, C, T], "classes": K, "dtype": "float64", "passes": passes}
    for name, run in (("tangent_space_fit_transform", lambda: rm.TangentSpace().fit_transform(cov)),
                      ("mdm_fit", lambda: rm.MDM().fit(cov, y))):
        for _ in range(warmup):
            run()
        wall, kern, calls = [], [], 0
        for _ in range(passes):
            torch.cuda.synchronize()
            with KernelClock() as kc:
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(kc.ms)
            calls = kc.calls
        line[f"{name}_wall_ms"] = round(float(np.median(wall)), 3)
        line[f"{name}_kernel_ms"] = round(float(np.median(kern)), 3)
        line[f"{name}_host_and_other_ms"] = round(float(np.median(wall) - np.median(kern)), 3)
        line[f"{name}_kernel_calls"] = calls
    _, it = rm.mean_riemann(cov, return_n_iter=True)
    _, its = rm.mean_riemann(cov, groups=y, return_n_iter=True)
    line.update(tangent_space_mean_iterations=int(it), mdm_mean_iterations=[int(v) for v in its],
                shader_clock_mhz=shader_clock_mhz())
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="350x64,4096x64,2048x128,4096x16", help="n x C stacks, comma separated")
    ap.add_argument("--no-pipeline", action="store_true")
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        n, C = (int(v) for v in shape.split("x"))
        bench_stack(n, C, a.passes, a.warmup)
    if not a.no_pipeline:
        bench_pipeline(a.passes, a.warmup)
    return 0


if __name__ == "__main__":
    sys.exit(main())
