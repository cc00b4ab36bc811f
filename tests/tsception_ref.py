"""Torch restatement of the reference's TSception (scripts/train_tsception.py:39-119, the published architecture:
multi-scale temporal convolutions + LeakyReLU + AvgPool + BatchNorm + FC).  It is the oracle of the TSception tests:
evaluated on the CPU in fp64 it is the reference value, in fp32 it measures how far one fp32 evaluation may sit from it.
Parity against the reference's own file is unpinned."""
import copy

import numpy as np
import torch
import torch.nn as nn


class TSception(nn.Module):
    def conv_block(self, i, o, k, s, pool):
        return nn.Sequential(nn.Conv2d(i, o, kernel_size=k, stride=s), nn.LeakyReLU(),
                             nn.AvgPool2d((1, pool), (1, pool)))

    def __init__(self, num_classes, input_size, sampling_rate, num_T, num_S, hidden, dropout_rate):
        super().__init__()
        win = [0.5, 0.25, 0.125]; pool = 8; C = input_size[1]            # input_size = (1, C, T)
        self.Tception1 = self.conv_block(1, num_T, (1, int(win[0] * sampling_rate)), 1, pool)
        self.Tception2 = self.conv_block(1, num_T, (1, int(win[1] * sampling_rate)), 1, pool)
        self.Tception3 = self.conv_block(1, num_T, (1, int(win[2] * sampling_rate)), 1, pool)
        self.Sception1 = self.conv_block(num_T, num_S, (int(C), 1), 1, int(pool * 0.25))
        self.Sception2 = self.conv_block(num_T, num_S, (int(C * 0.5), 1), (int(C * 0.5), 1), int(pool * 0.25))
        self.fusion_layer = self.conv_block(num_S, num_S, (3, 1), 1, 4)
        self.BN_t = nn.BatchNorm2d(num_T); self.BN_s = nn.BatchNorm2d(num_S); self.BN_fusion = nn.BatchNorm2d(num_S)
        self.fc = nn.Sequential(nn.Linear(num_S, hidden), nn.ReLU(), nn.Dropout(dropout_rate),
                                nn.Linear(hidden, num_classes))

    def forward(self, x):                                                # x [B, 1, C, T]
        out = torch.cat([self.Tception1(x), self.Tception2(x), self.Tception3(x)], dim=-1)
        out = self.BN_t(out)
        out = torch.cat([self.Sception1(out), self.Sception2(out)], dim=2)
        out = self.BN_s(out)
        out = self.fusion_layer(out)
        out = self.BN_fusion(out)
        out = torch.squeeze(torch.mean(out, dim=-1), dim=-1)
        return self.fc(out)


# ----------------------------------------------------------------------------- helpers of the tests
def make_ref(C, T, fs, num_T, num_S, hidden, n_classes=5, seed=0, dropout=0.0):
    """An fp32 restatement on the CPU whose BatchNorm weights ~ U(0.5, 1.5) and biases ~ U(-0.3, 0.3) matter."""
    torch.manual_seed(seed)
    m = TSception(n_classes, (1, C, T), fs, num_T, num_S, hidden, dropout)
    with torch.no_grad():
        for bn in (m.BN_t, m.BN_s, m.BN_fusion):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.3, 0.3)
    return m


def as_double(m):
    return copy.deepcopy(m).double()


class FixedMask(nn.Module):
    """nn.Dropout with a given keep mask [B, units]."""

    def __init__(self, keep, p):
        super().__init__()
        self.keep, self.p = keep, p

    def forward(self, h):
        return h * self.keep.to(h.dtype) / (1.0 - self.p)


def train_pass(m, x, w):
    """Train-mode forward and backward of ``loss = (logits * w).sum()`` on a copy of ``m`` in its own dtype:
    (logits, {name: grad}, {buffer name: value})."""
    m = copy.deepcopy(m).train()
    dt = next(m.parameters()).dtype
    logits = m(x.to(dt)[:, None])
    (logits * w.to(dt)).sum().backward()
    grads = {k: p.grad.detach().double() for k, p in m.named_parameters()}
    bufs = {k: v.detach().clone() for k, v in m.named_buffers()}
    return logits.detach().double(), grads, bufs


def grad_errors(got, want):
    """Per-parameter  max |got - want| / max(max |want|, 1e-3 * largest gradient magnitude)."""
    scale = max(float(v.abs().max()) for v in want.values())
    return {k: float((got[k].double().cpu() - want[k]).abs().max()) / max(float(want[k].abs().max()), 1e-3 * scale)
            for k in want}


def bound(deviation):
    """The tolerance rule: max(1e-4, 4 x the fp32 restatement's own deviation), refusing a badly conditioned case."""
    assert 4.0 * deviation <= 5e-4, f"badly conditioned: the fp32 restatement itself deviates by {deviation:.2e}"
    return max(1e-4, 4.0 * deviation)


def class_tone_trials(n, C, T, fs, seed, n_classes=5):
    """SURVEY.md 8(d) synthetic task at a small montage: unit white noise + 0.5 sin(2 pi f_y t + phi) on the channels
    c with c % n_classes == y."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, C, T), dtype=np.float32)
    y = rng.integers(0, n_classes, n).astype(np.int64)
    tone = np.array([6.0, 10.0, 18.0, 26.0, 34.0])[:n_classes] * (fs / 256.0)
    phase = rng.uniform(0.0, 2.0 * np.pi, n)
    t = np.arange(T) / fs
    for i in range(n):
        ch = [c for c in range(C) if c % n_classes == y[i]]
        X[i, ch] += (0.5 * np.sin(2.0 * np.pi * tone[y[i]] * t + phase[i])).astype(np.float32)
    return X, y
