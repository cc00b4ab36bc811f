"""Expected-gradients attributions (isd_amd.explain.GradientExplainer): where the time goes.

Two model families, n = 64 trials, S = 200 draws, K = 5 classes, tiles of 256 pairs:
  cfg2: FilterbankCNNClassifier on 64 x 512 trials, 9 bands;   fast: nn.FAST 'default' on 64 x 800 trials.
Per family, one JSON line: total time of shap_values, time inside isd_attr_mix / isd_attr_accumulate (device events
around every call), their algorithmic bytes and the achieved fraction of the 6.3 TB/s a float4 copy reaches (DESIGN.md
3.1), peak device memory of the call against the n*S*E*4 bytes of one materialised interpolant, and the sampling
arithmetic alone -- mix + K accumulates per tile on a fixed gradient buffer -- against the same arithmetic in torch ops
(index_select / lerp / (x - b) * g / index_add_), alternating in one process, median of the passes.
Exits non-zero if the kernels are slower than the torch composition or the peak memory reaches the interpolant's."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import isd_amd
from isd_amd import explain as ex

COPY_BYTES_PER_S = 6.3e12


def make_cfg2(dev):
    X = torch.randn(32, 64, 512, device=dev)
    y = torch.randint(0, 5, (32,), device=dev)
    clf = isd_amd.FilterbankCNNClassifier(max_epochs=1, batch_size=16, warmup_epochs=0)
    clf.fit(X, y)
    return clf, (64, 512)


def make_fast(dev):
    import isd_amd.nn as inn
    torch.manual_seed(0)
    return inn.FAST(inn.fast_config()).to(dev), (64, 800)


class KernelClock:
    """Device events around every isd_attr_* call of the explainer, and the bytes each call has to move."""

    def __init__(self):
        self.events = {"mix": [], "accumulate": []}
        self.bytes = {"mix": 0, "accumulate": 0}
        self._mix, self._acc = ex.attr_mix, ex.attr_accumulate

    def __enter__(self):
        def trials(p0, m, S):
            return (p0 + m - 1) // S - p0 // S + 1

        def mix(x, bg, ridx, alpha, out, p0, m, S):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self._mix(x, bg, ridx, alpha, out, p0, m, S)
            e1.record()
            self.events["mix"].append((e0, e1))
            self.bytes["mix"] += (trials(p0, m, S) + 2 * m) * x.shape[-1] * 4      # x per trial, bg + out per pair
            return out

        def acc(x, bg, ridx, grad, a, p0, m, S, scale):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self._acc(x, bg, ridx, grad, a, p0, m, S, scale)
            e1.record()
            self.events["accumulate"].append((e0, e1))
            self.bytes["accumulate"] += (2 * m + 3 * trials(p0, m, S)) * x.shape[-1] * 4   # grad + bg per pair; x, acc
            return a
        ex.attr_mix, ex.attr_accumulate = mix, acc
        return self

    def __exit__(self, *exc):
        ex.attr_mix, ex.attr_accumulate = self._mix, self._acc

    def ms(self, which):
        return sum(a.elapsed_time(b) for a, b in self.events[which])


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def sampling_arithmetic(n, S, K, E, M, bs, passes, dev):
    """mix + K accumulates per tile on a fixed gradient buffer: the HIP kernels against torch ops, alternating."""
    x, bg = torch.randn(n, E, device=dev), torch.randn(M, E, device=dev)
    ridx_h, alpha_h = ex.draw_samples(n, S, M, 0)
    ridx = torch.as_tensor(ridx_h).to(dev).reshape(-1)
    alpha = torch.as_tensor(alpha_h).to(dev).reshape(-1)
    trial = torch.arange(n, device=dev).repeat_interleave(S)
    g = torch.randn(bs, E, device=dev)
    buf = torch.empty(bs, E, device=dev)
    acc = torch.zeros(K, n, E, device=dev)
    n_pairs = n * S

    def hip():
        acc.zero_()
        for p0 in range(0, n_pairs, bs):
            m = min(bs, n_pairs - p0)
            ex.attr_mix(x, bg, ridx, alpha, buf, p0, m, S)
            for k in range(K):
                ex.attr_accumulate(x, bg, ridx, g[:m], acc[k], p0, m, S, 1.0 / S)

    def torch_ops():
        acc.zero_()
        for p0 in range(0, n_pairs, bs):
            m = min(bs, n_pairs - p0)
            ti, r = trial[p0:p0 + m], ridx[p0:p0 + m].long()
            xi, b = x.index_select(0, ti), bg.index_select(0, r)
            torch.lerp(b, xi, alpha[p0:p0 + m, None], out=buf[:m])
            for k in range(K):
                acc[k].index_add_(0, ti, (xi - b) * g[:m])
        acc.mul_(1.0 / S)

    hip(), torch_ops()
    torch.cuda.synchronize()
    th, tt = [], []
    for _ in range(passes):
        th.append(timed(hip))
        tt.append(timed(torch_ops))
    return float(np.median(th)), float(np.median(tt)), th, tt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", default="cfg2,fast")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--nsamples", type=int, default=200)
    ap.add_argument("--background", type=int, default=32)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    ok = True
    for fam in a.families.split(","):
        model, (Cc, T) = {"cfg2": make_cfg2, "fast": make_fast}[fam](dev)
        n, S, M, E = a.n, a.nsamples, a.background, Cc * T
        X, bg = torch.randn(n, Cc, T, device=dev), torch.randn(M, Cc, T, device=dev)
        explainer = ex.GradientExplainer(model, bg, batch_size=a.batch_size)
        explainer.shap_values(X[:2], nsamples=max(a.batch_size // 2, 1))           # warm-up: plans, workspaces
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with KernelClock() as clock:
            out = {}
            total = timed(lambda: out.setdefault("phi", explainer.shap_values(X, nsamples=S)))
        peak = torch.cuda.max_memory_allocated() - base
        K = out["phi"].shape[-1]
        interp = n * S * E * 4
        hip_ms, torch_ms, th, tt = sampling_arithmetic(n, S, K, E, M, a.batch_size, a.passes, dev)
        line = {"family": fam, "n": n, "S": S, "K": K, "E": E, "batch_size": a.batch_size, "total_ms": round(total, 2)}
        for which in ("mix", "accumulate"):
            ms = clock.ms(which)
            line[f"{which}_ms"] = round(ms, 3)
            line[f"{which}_GB"] = round(clock.bytes[which] / 1e9, 3)
            line[f"{which}_fraction_of_copy_rate"] = round(clock.bytes[which] / (ms * 1e-3) / COPY_BYTES_PER_S, 3)
        line["kernels_share_of_total"] = round((clock.ms("mix") + clock.ms("accumulate")) / total, 4)
        line.update(peak_extra_MiB=round(peak / 2 ** 20, 1), interpolant_MiB=round(interp / 2 ** 20, 1),
                    sampling_hip_ms=round(hip_ms, 3), sampling_torch_ms=round(torch_ms, 3),
                    sampling_torch_over_hip=round(torch_ms / hip_ms, 2),
                    sampling_hip_ms_all=[round(v, 3) for v in th], sampling_torch_ms_all=[round(v, 3) for v in tt])
        line["ok"] = bool(hip_ms <= torch_ms and peak < interp)
        ok &= line["ok"]
        print(json.dumps(line), flush=True)
        del model, explainer
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
