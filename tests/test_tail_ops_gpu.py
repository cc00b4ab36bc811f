"""The per-operator transformer tail against fp64: the autograd functions of isd_amd.nn on csrc/tail.hip (embed,
LayerNorm, attention core) and csrc/fc.hip (linear, linear + residual, softmax cross-entropy), one operator at a time
and as the whole tail of a FAST model that the fused kernel (csrc/tailfused.hip) does not serve.  The reference is
tests/tail_ref.py on the fp32 inputs widened to fp64; gradients come from autograd over it.

Bounds.  rel_err (max-abs over the reference's max-abs) < 1e-5 for every operator on unit-scale inputs, the bound of
test_linear_forward_backward_vs_torch; whole tail: logits 1e-4, gradients 2e-4, the bounds of test_tail_fused_gpu.py.
On the stress inputs fp32's own error is set by the input, so the bound is taken from the reference side: the same
operation in torch fp32 on the CPU is compared with fp64, and the kernel may err four times as much (its sums run in
another order), never less than 1e-5.  Both figures are printed.  Measured on an MI355X, each against fp64, the
largest over the cases with D > 1 (at D = 1 the reference gradients are exactly zero, and so are the kernel's):

                                           kernel                     torch fp32 (CPU)
    LayerNorm, rows offset by 1e3          y 1.3e-7  dx 1.8e-7        y 1.0e-6 .. 1.1e-4   dx 4.3e-6 .. 2.4e-4
                                           dw 1.6e-7 db 1.2e-7        dw 1.1e-6 .. 1.3e-4  db 2.9e-7
    LayerNorm, rows of std 1e-3            y 6.9e-8  dx 2.1e-7        y 7.8e-8   dx 1.9e-7
      (eps 1e-5 and 1e-3)                  dw 2.0e-7 db 1.2e-7        dw 2.0e-7  db 2.9e-7
    attention, qkv * 6                     ctx 1.2e-6  dqkv 9.6e-7    ctx 7.4e-7  dqkv 9.6e-7
                                           probs 1.5e-6               probs 8.7e-7
    cross-entropy, logits * 40             loss 5.3e-8  dlogits 2.0e-6  loss 5.3e-8  dlogits 8.1e-7

torch's error on the offset rows varies 100-fold from case to case, so the bound does too; where it is smallest
(D = 33, M = 1: y 1.0e-6, i.e. the 1e-5 floor) a LayerNorm that centres a row with a one-word fp32 mean misses it:
the kernel did (y 2.5e-5 there, dw 9.1e-5 against a bound of 3.9e-5 at D = 48, M = 1) until it kept the mean in two
words (csrc/tail.hip, layernorm_fwd_kernel).
"""
import pytest
import torch
import torch.nn.functional as F

import tail_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope="module")
def inn():
    import isd_amd.nn as m
    assert torch.cuda.is_available()
    return m


def _leaves(ts, dtype, device="cpu"):
    return [None if t is None else t.detach().to(device=device, dtype=dtype).requires_grad_(t.is_floating_point())
            for t in ts]


def _run(fn, ts, dy, dtype, device="cpu"):
    """fn(*leaves) and the gradients of sum(y * dy) -> [y, grad of every floating-point leaf] on the CPU."""
    leaves = _leaves(ts, dtype, device)
    y = fn(*leaves)
    (y * dy.to(device=device, dtype=dtype)).sum().backward()
    return [y.detach().cpu()] + [t.grad.detach().cpu() for t in leaves if t is not None and t.requires_grad]


def _compare(tag, names, got, want, bad, got32=None):
    """Every quantity of ``got`` against ``want`` (fp64) under 1e-5, or -- stress inputs, ``got32`` the same operation
    in torch fp32 on the CPU -- under four times fp32's own error, at least 1e-5.  Misses are collected in ``bad``."""
    assert len(got) == len(want) == len(names), tag
    for i, (n, g, w) in enumerate(zip(names, got, want)):
        assert g.shape == w.shape, (tag, n)
        if w.numel() == 0:
            continue
        assert bool(torch.isfinite(g).all()), (tag, n)
        e, bnd = rel_err(g, w), TOL
        if got32 is not None:
            e32 = rel_err(got32[i], w)
            bnd = max(4.0 * e32, TOL)
            print(f"{tag} {n}: kernel {e:.2e}  torch fp32 {e32:.2e}  bound {bnd:.2e}")
        if not e < bnd:
            bad.append((tag, n, e, bnd))


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("M", [1, 3, 5, 1025])      # a lone row, a partial workgroup, one row past it, a strided wgrad
@pytest.mark.parametrize("D", [1, 7, 33, 48, 64])
def test_layer_norm_vs_fp64(inn, D, M):
    gen = torch.Generator().manual_seed(1000 * D + M)
    n = torch.randn(M, D, generator=gen)
    w = 0.5 + torch.rand(D, generator=gen)
    b = torch.randn(D, generator=gen)
    dy = torch.randn(M, D, generator=gen)
    names = ("y", "dx", "dw", "db")
    bad = []
    for family, x, eps, stress in (("unit", n, 1e-5, False), ("std1e-3", 1e-3 * n, 1e-5, True),
                                   ("std1e-3", 1e-3 * n, 1e-3, True), ("offset1e3", n + 1e3, 1e-5, True)):
        want = _run(lambda x_, w_, b_: R.layer_norm(x_, w_, b_, eps), (x, w, b), dy, torch.float64)
        got32 = None
        if stress:
            got32 = _run(lambda x_, w_, b_: F.layer_norm(x_, (D,), w_, b_, eps), (x, w, b), dy, torch.float32)
        got = _run(lambda x_, w_, b_: inn.layer_norm(x_, w_, b_, eps), (x, w, b), dy, torch.float32, "cuda")
        _compare(f"layer_norm D={D} M={M} {family} eps={eps:g}", names, got, want, bad, got32)
    assert not bad, bad


def test_layer_norm_zero_row_is_the_bias_and_wide_rows_are_refused(inn):
    import isd_amd._lib as L
    gen = torch.Generator().manual_seed(3)
    for D in (1, 7, 33, 48, 64):
        w, b = (0.5 + torch.rand(D, generator=gen)).cuda(), torch.randn(D, generator=gen).cuda()
        x = torch.randn(6, D, generator=gen).cuda()
        x[1] = 0.0
        x[5] = 0.0
        y = inn.layer_norm(x, w, b, 1e-5)
        assert torch.equal(y[1], b) and torch.equal(y[5], b), D
    with pytest.raises(L.IsdError, match="isd_layernorm_forward"):
        inn.layer_norm(torch.randn(3, 65, device="cuda"), torch.ones(65, device="cuda"), torch.zeros(65, device="cuda"))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ attention core
def _attention_case(B, S, H, dh, scale=1.0):
    gen = torch.Generator().manual_seed(B * 1000 + S * 100 + H * 10 + dh)
    return scale * torch.randn(B, S, 3 * H * dh, generator=gen), torch.randn(B, S, H * dh, generator=gen)


def _attention_gpu(inn, qkv, dctx, H, p, seed):
    """-> [ctx, dqkv, probs as saved for the backward pass] on the CPU."""
    q = qkv.cuda().requires_grad_()
    out = inn._AttentionFn.apply(q, H, p, seed)
    probs = out.grad_fn.saved_tensors[1].detach().cpu().clone()
    (out * dctx.cuda()).sum().backward()
    return [out.detach().cpu(), q.grad.cpu(), probs]


def _attention_ref(qkv, dctx, H, dtype, mask=None, p=0.0):
    q = qkv.detach().to(dtype).requires_grad_()
    ctx, probs = R.attention(q, H, mask, p)
    (ctx * dctx.to(dtype)).sum().backward()
    return [ctx.detach(), q.grad, probs.detach()]


@pytest.mark.parametrize("B,S,H,dh", [(1, 1, 1, 1), (3, 8, 8, 8), (5, 6, 3, 5), (2, 7, 1, 8), (300, 3, 2, 4)])
def test_attention_vs_fp64(inn, B, S, H, dh):
    qkv, dctx = _attention_case(B, S, H, dh)
    bad = []
    _compare(f"attention {(B, S, H, dh)}", ("ctx", "dqkv", "probs"), _attention_gpu(inn, qkv, dctx, H, 0.0, 0),
             _attention_ref(qkv, dctx, H, torch.float64), bad)
    assert not bad, bad


def test_attention_large_logits(inn):
    """qkv * 6: logits near +-35, so the softmax lives on its max subtraction."""
    B, S, H, dh = 3, 8, 8, 8
    qkv, dctx = _attention_case(B, S, H, dh, 6.0)
    want = _attention_ref(qkv, dctx, H, torch.float64)
    q, k = (qkv[..., t * H * dh:(t + 1) * H * dh].reshape(B, S, H, dh).transpose(1, 2).double() for t in range(2))
    assert float((q @ k.transpose(-1, -2)).abs().max()) / dh ** 0.5 > 35.0
    bad = []
    _compare("attention qkv*6", ("ctx", "dqkv", "probs"), _attention_gpu(inn, qkv, dctx, H, 0.0, 0), want, bad,
             _attention_ref(qkv, dctx, H, torch.float32))
    assert not bad, bad


# (B, S, H, head_dim); the last is the second with S and H exchanged: 540 mask elements rather than 270
@pytest.mark.parametrize("B,S,H,dh", [(3, 8, 8, 8), (5, 3, 6, 6), (5, 6, 3, 6)])
def test_attention_dropout_matches_the_host_mask(inn, B, S, H, dh):
    p, seed = 0.3, 12345
    qkv, dctx = _attention_case(B, S, H, dh)
    mask = R.drop_keep_mask(seed, (B, H, S, S), p)
    kept = float(mask.mean())
    print(f"kept share {kept:.3f} over {mask.numel()} elements")
    assert abs(kept - 0.70) <= 0.05
    want = _attention_ref(qkv, dctx, H, torch.float64, mask, p)      # want[2]: the softmax before dropout
    got = _attention_gpu(inn, qkv, dctx, H, p, seed)
    bad = []
    _compare(f"attention dropout {(B, S, H, dh)}", ("ctx", "dqkv", "probs"), got, want, bad)
    assert not bad, bad
    again = _attention_gpu(inn, qkv, dctx, H, p, seed)
    assert all(torch.equal(a, g) for a, g in zip(again, got))
    other = _attention_gpu(inn, qkv, dctx, H, p, seed + 1)
    assert not torch.equal(other[0], got[0]) and not torch.equal(other[1], got[1])
    assert torch.equal(other[2], got[2])                             # the saved softmax does not depend on the mask
    clean = _attention_ref(qkv, dctx, H, torch.float64)
    assert rel_err(got[0], clean[0]) > 1e-2                          # and the mask was applied at all


def test_attention_refuses_shapes_outside_its_arrays(inn):
    import isd_amd._lib as L
    for (S, H, dh, p), what in (((9, 2, 4, 0.0), "isd_attention_forward: S=9"),
                                ((4, 2, 9, 0.0), "head_dim=9"), ((4, 2, 4, 1.0), "dropout_p")):
        with pytest.raises(L.IsdError, match=what):
            inn._AttentionFn.apply(torch.randn(2, S, 3 * H * dh, device="cuda"), H, p, 1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ cls / positional embedding
@pytest.mark.parametrize("B,N,D", [(1, 0, 16), (3, 1, 1), (5, 7, 33), (300, 5, 64)])
def test_embed_vs_fp64(inn, B, N, D):
    gen = torch.Generator().manual_seed(B + N + D)
    x, cls, pos = torch.randn(B, N, D, generator=gen), torch.randn(1, 1, D, generator=gen), \
        torch.randn(1, N + 1, D, generator=gen)
    dtok = torch.randn(B, N + 1, D, generator=gen)
    want = _run(R.embed, (x, cls, pos), dtok, torch.float64)
    got = _run(inn._EmbedFn.apply, (x, cls, pos), dtok, torch.float32, "cuda")
    assert got[1].shape == (B, N, D)                                 # N = 0: a gradient for cls and pos only
    bad = []
    _compare(f"embed {(B, N, D)}", ("tok", "dx", "dcls", "dpos"), got, want, bad)
    assert not bad, bad


# ------------------------------------------------------------------ linear, linear + residual
LINEAR_CASES = [(1, 1, 1), (37, 64, 64), (65, 70, 33), (17, 257, 96), (130, 300, 65), (70, 1000, 192), (4100, 32, 64)]


def _linear_case(M, K, N):
    gen = torch.Generator().manual_seed(M + K + N)
    return (torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) / K ** 0.5, torch.randn(N, generator=gen),
            torch.randn(M, N, generator=gen), torch.randn(M, N, generator=gen))


@pytest.mark.parametrize("M,K,N", LINEAR_CASES)
def test_linear_vs_fp64(inn, M, K, N):
    x, w, b, _, dy = _linear_case(M, K, N)
    bad = []
    for act in (False, True):
        for bias in (b, None):
            names = ("y", "dx", "dw") + (("db",) if bias is not None else ())
            want = _run(lambda x_, w_, b_: R.linear(x_, w_, b_, act), (x, w, bias), dy, torch.float64)
            got = _run(lambda x_, w_, b_: inn.linear(x_, w_, b_, act=act), (x, w, bias), dy, torch.float32, "cuda")
            _compare(f"linear {(M, K, N)} act={act} bias={bias is not None}", names, got, want, bad)
    assert not bad, bad


@pytest.mark.parametrize("M,K,N", LINEAR_CASES)
def test_linear_residual_vs_fp64(inn, M, K, N):
    x, w, b, res, dy = _linear_case(M, K, N)
    want = _run(R.linear_residual, (x, w, b, res), dy, torch.float64)
    got = _run(inn.linear_residual, (x, w, b, res), dy, torch.float32, "cuda")
    bad = []
    _compare(f"linear_residual {(M, K, N)}", ("y", "dx", "dw", "db", "dres"), got, want, bad)
    assert not bad, bad


# ------------------------------------------------------------------ token-mean cross-entropy and predict
def _ce_case(B, n_tok, n_cls, scale=1.0):
    gen = torch.Generator().manual_seed(B + n_tok + n_cls)
    return scale * torch.randn(B, n_tok, n_cls, generator=gen), torch.randint(0, n_cls, (B,), generator=gen)


def _ce_ref(lt, y, dtype, global_batch=None, fn=R.token_mean_cross_entropy):
    l = lt.detach().to(dtype).requires_grad_()
    loss = fn(l, y, global_batch)
    loss.backward()
    return [loss.detach().reshape(1), l.grad]


def _ce_gpu(inn, lt, y, global_batch=None):
    l = lt.cuda().requires_grad_()
    loss = inn.token_mean_cross_entropy(l, y.cuda(), global_batch)
    loss.backward()
    return [loss.detach().cpu().reshape(1), l.grad.cpu()]


@pytest.mark.parametrize("labels", [torch.uint8, torch.int64])
@pytest.mark.parametrize("B,n_tok,n_cls", [(3, 1, 32), (300, 4, 17), (257, 1, 1)])
def test_softmax_ce_vs_fp64(inn, B, n_tok, n_cls, labels):
    lt, y = _ce_case(B, n_tok, n_cls)
    y = y.to(labels)
    want = _ce_ref(lt, y, torch.float64)
    got = _ce_gpu(inn, lt, y)
    bad = []
    _compare(f"softmax_ce {(B, n_tok, n_cls)}", ("loss", "dlogits"), got, want, bad)
    half = _ce_gpu(inn, lt, y, 2 * B)                                # the share of a global batch twice as large
    _compare("global_batch=2B", ("loss", "dlogits"), half, [0.5 * t for t in want], bad)
    assert torch.equal(half[0] * 2, got[0]) and torch.equal(half[1] * 2, got[1])
    lm, pred = inn.token_mean_predict(lt.cuda())
    _compare("token_mean_predict", ("mean",), [lm.cpu()], [lt.double().mean(1)], bad)
    assert torch.equal(pred.cpu(), torch.argmax(lm.cpu(), dim=1))    # ties -> lowest index, on the kernel's own means
    top = lt.double().mean(1).topk(min(2, n_cls), dim=1).values
    clear = (top[:, 0] - top[:, -1] > 1e-4) if n_cls > 1 else torch.ones(B, dtype=torch.bool)
    assert torch.equal(pred.cpu()[clear], torch.argmax(lt.double().mean(1), dim=1)[clear])
    assert not bad, bad


def test_softmax_ce_large_logits_and_class_limit(inn):
    import isd_amd._lib as L
    lt, y = _ce_case(300, 4, 17, 40.0)
    want = _ce_ref(lt, y, torch.float64)
    got32 = _ce_ref(lt, y, torch.float32, fn=lambda l, y_, _: F.cross_entropy(l.mean(1), y_))
    bad = []
    _compare("softmax_ce logits*40", ("loss", "dlogits"), _ce_gpu(inn, lt, y), want, bad, got32)
    assert not bad, bad
    with pytest.raises(L.IsdError, match="isd_softmax_ce"):
        inn.token_mean_cross_entropy(torch.randn(4, 1, 33, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"))
    with pytest.raises(L.IsdError, match="isd_softmax_ce"):
        inn.token_mean_predict(torch.randn(4, 1, 33, device="cuda"))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the whole tail on the per-operator route
@pytest.mark.parametrize("B,N,kw,eps", [
    (5, 5, dict(dim_token=64, num_heads=8), 1e-5),                                     # D = 64: in_proj is 192 wide
    (9, 2, dict(dim_token=48, num_heads=6, num_layers=2), 1e-5),                       # D = 48, head width 8
    (4, 7, dict(dim_token=40, num_heads=8, num_layers=1, n_classes=3, seq_len=1000), 1e-5),   # head width 5, 8 tokens
    (5, 5, {}, 1e-3),                                                                  # production shape, another eps
    (3, 0, dict(dim_token=64, num_heads=8), 1e-5),                                     # the cls token alone
])
def test_per_operator_tail_vs_fp64(inn, B, N, kw, eps):
    torch.manual_seed(100 + B + N)
    m = inn.FAST(inn.fast_config(dropout=0.0, **kw)).cuda().train()
    for blk in m.transformer:
        blk.layer_norm_1.eps = blk.layer_norm_2.eps = eps
    c = m.config
    assert N <= m.n_tokens
    assert not m._tail_fusable(torch.zeros(B, N, c.dim_token, device="cuda"))         # never the fused kernel
    feature = torch.randn(B, N, 8, 32, device="cuda")
    y = torch.randint(0, c.n_classes, (B,), device="cuda")
    want, p = R.torch_tail(m, feature, eps)
    F.cross_entropy(want, y.cpu()).backward()
    f = feature.clone().requires_grad_()
    logits = m.forward_transformer(f)
    assert logits.shape == (B, c.n_classes)
    assert rel_err(logits.detach().cpu(), want.detach()) < 1e-4
    if eps != 1e-5:                                                  # a dropped eps cannot pass
        other, _ = R.torch_tail(m, feature, 1e-5)
        assert rel_err(logits.detach().cpu(), other.detach()) > 1e-4
    F.cross_entropy(logits, y).backward()
    named = {k: q for k, q in m.named_parameters() if not k.startswith("head.")}
    assert len(named) == 2 + 2 + 2 + 12 * len(m.transformer)
    bad = [(k, e) for k, e in ((k, rel_err(q.grad.cpu(), p[k].grad)) for k, q in named.items()) if not e < 2e-4]
    assert not bad, bad
    if N:
        assert rel_err(f.grad.cpu().reshape(B, N, -1), p["feature"].grad) < 2e-4
    else:
        assert f.grad is None or f.grad.numel() == 0
    m.eval()                                                         # inference runs the same kernels
    with torch.no_grad():
        assert torch.equal(m.forward_transformer(feature), logits.detach())


def test_per_operator_tail_refuses_nine_tokens(inn):
    import isd_amd._lib as L
    m = inn.FAST(inn.fast_config(dropout=0.0, seq_len=1250)).cuda()
    assert m.n_tokens == 9
    assert not m._tail_fusable(torch.zeros(2, 8, 32, device="cuda"))
    with pytest.raises(L.IsdError, match="isd_attention_forward: S=9"):
        m.forward_transformer(torch.randn(2, 8, 8, 32, device="cuda"))            # cls + 8 windows
    torch.cuda.synchronize()                                         # refused by the argument check: nothing was launched
    assert m.forward_transformer(torch.randn(2, 7, 8, 32, device="cuda")).shape == (2, 5)
