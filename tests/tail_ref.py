"""Plain torch restatement of the per-operator transformer tail (isd_amd/nn.py on csrc/tail.hip and csrc/fc.hip),
independent of the package: LayerNorm, the attention core on packed qkv, the cls / positional embedding, the dense
layers, the token-mean cross-entropy, and the whole tail of fast.py:260-268 on the stock torch modules.  Every function
computes in the dtype of its arguments: the tests widen the fp32 inputs to fp64 for the reference (gradients come from
autograd over these functions) and run the same functions in fp32 where a bound is taken from fp32's own error.
`drop_keep_mask` restates the counter-based attention dropout mask of csrc/tail.hip (tail_drop_scale) on uint64.
Shared by test_tail_ops_gpu.py and test_tail_fused_gpu.py."""
import numpy as np
import torch
import torch.nn.functional as F


def layer_norm(x, w, b, eps):
    """nn.LayerNorm over the last dim: biased variance, eps inside the square root."""
    mu = x.mean(-1, keepdim=True)
    c = x - mu
    var = (c * c).mean(-1, keepdim=True)
    return c / torch.sqrt(var + eps) * w + b


def attention(qkv, H, mask=None, p=0.0):
    """qkv [B, S, 3D] (q | k | v, heads contiguous inside each) -> (ctx [B, S, D], probs [B, H, S, S]); probs is the
    softmax before dropout.  ``mask`` [B, H, S, S] of 0 / 1 is applied as probs * mask / (1 - p)."""
    B, S, D3 = qkv.shape
    D = D3 // 3
    dh = D // H
    q, k, v = (qkv[..., t * D:(t + 1) * D].reshape(B, S, H, dh).transpose(1, 2) for t in range(3))     # [B, H, S, dh]
    probs = torch.softmax(q @ k.transpose(-1, -2) / dh ** 0.5, dim=-1)
    pd = probs if mask is None else probs * mask.to(probs.dtype) / (1.0 - p)
    return (pd @ v).transpose(1, 2).reshape(B, S, D), probs


def embed(x, cls, pos):
    """tokens = cat(cls, x) + pos[:, :N + 1]   (x [B, N, D], cls [1, 1, D], pos [1, >= N + 1, D])."""
    B, N, _ = x.shape
    return torch.cat([cls.expand(B, -1, -1), x], dim=1) + pos[:, :N + 1]


def linear(x, w, b=None, act=False):
    y = x @ w.T
    if b is not None:
        y = y + b
    return 0.5 * y * (1.0 + torch.erf(y * 0.5 ** 0.5)) if act else y


def linear_residual(x, w, b, res):
    return x @ w.T + b + res


def token_mean_cross_entropy(logits_tok, labels, global_batch=None):
    """CrossEntropyLoss()(logits_tok.mean(1), labels) * B / global_batch   (logits_tok [B, n_tok, n_cls])."""
    lm = logits_tok.mean(1)
    B = lm.shape[0]
    nll = torch.logsumexp(lm, dim=-1) - lm.gather(1, labels.long().view(B, 1))[:, 0]
    return nll.sum() / float(global_batch or B)


def drop_keep_mask(seed, shape, p):
    """tail_drop_scale of csrc/tail.hip on the host: the 0 / 1 keep-mask over probs [B, H, S, S] (float64 tensor).
    Element idx (flat index) is kept when u >= float32(p), u = float32(v >> 40) * 2^-24, v the splitmix64 finaliser of
    (idx + golden ratio) ^ seed."""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        v = (np.arange(n, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(seed)
        v ^= v >> np.uint64(30)
        v *= np.uint64(0xBF58476D1CE4E5B9)
        v ^= v >> np.uint64(27)
        v *= np.uint64(0x94D049BB133111EB)
        v ^= v >> np.uint64(31)
    u = (v >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    return torch.from_numpy((u >= np.float32(p)).astype(np.float64).reshape(shape))


def torch_tail(m, feature, eps=1e-5):
    """fast.py:260-268 with the stock torch modules on the parameters of ``m`` (fp64 on the CPU), every LayerNorm with
    ``eps``.  -> (logits, p): p maps the parameter names to the fp64 leaves, and "feature" to the [B, N, Z * F] input
    leaf, so that after a backward pass p[k].grad is the reference gradient."""
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    p = {k: v.clone().requires_grad_() for k, v in sd.items()}
    B, N, Z, Fd = feature.shape
    x = feature.detach().cpu().double().reshape(B, N, Z * Fd).requires_grad_()
    p["feature"] = x
    tok = F.gelu(F.linear(x, p["input_layer.0.weight"], p["input_layer.0.bias"]))
    tok = torch.cat([p["cls_token"].expand(B, -1, -1), tok], dim=1) + p["pos_embedding"][:, :N + 1]
    D, H = m.config.dim_token, m.config.num_heads
    for l in range(len(m.transformer)):
        q = f"transformer.{l}."
        h = F.layer_norm(tok, (D,), p[q + "layer_norm_1.weight"], p[q + "layer_norm_1.bias"], eps)
        a, _ = F.multi_head_attention_forward(
            h.transpose(0, 1), h.transpose(0, 1), h.transpose(0, 1), D, H, p[q + "attn.in_proj_weight"],
            p[q + "attn.in_proj_bias"], None, None, False, 0.0, p[q + "attn.out_proj.weight"],
            p[q + "attn.out_proj.bias"], training=False, need_weights=False)
        tok = tok + a.transpose(0, 1)
        h = F.layer_norm(tok, (D,), p[q + "layer_norm_2.weight"], p[q + "layer_norm_2.bias"], eps)
        h = F.gelu(F.linear(h, p[q + "linear.0.weight"], p[q + "linear.0.bias"]))
        tok = tok + F.linear(h, p[q + "linear.3.weight"], p[q + "linear.3.bias"])
    return F.linear(tok[:, 0], p["last_layer.weight"], p["last_layer.bias"]), p
