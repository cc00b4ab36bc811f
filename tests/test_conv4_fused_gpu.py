"""GPU: the fused Conv4Layers kernels (conv4_fused_fwd_kernel / conv4_fused_bwd_kernel and their bf16 twins,
csrc/conv.hip) against the fp64 oracle where the reference zones never take them: a zone of 16 channels (the widest
the fused routes admit -- the last x row is the neighbour of the first activation tile in LDS), more items than
persistent workgroups (the one-item-ahead x prefetch, weight gradients accumulated over a workgroup's items), zones of
16 / 13 / 12 / 1 gathered channels in one launch, and every boundary of the window length: TT = 4 and 16 column
tiles, a ragged last tile, either side of the fifth 64-step chunk of the x fetch.

Every case asserts the route through isd_first_layer_last_path (6 = conv4_fused_fwd_kernel, 7 =
conv4_fused_fwd_bf16_kernel): a fall-back to the layer-wise chain cannot pass for the fused kernels.  The oracle
results are computed once per shape and shared by the tests that need them.
"""
import functools

import pytest
import torch

from conftest import rel_err
from oracle import cnn as ocnn

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the fused fp32 route against fp64, as in test_cnn_gpu.py
FUSED_F32, FUSED_BF16 = 6, 7


@pytest.fixture(scope="module")
def inn():
    import isd_amd.nn as m
    assert torch.cuda.is_available()
    return m


def _fwd_path():
    """Forward code of the calling thread's last isd_conv4_forward (the low four bits)."""
    from isd_amd import _lib
    return _lib.lib().isd_first_layer_last_path() & 15


# ------------------------------------------------------------------ (a) one zone of 16 channels
# window lengths: 53 (TT = 4, the route's lower bound), 57 (T1 = 53: ragged last column tile), 250 (the reference
# window, T1 = 246), 256 / 257 (the x fetch takes its fifth 64-step chunk from 257 on), 260 (TT = 16, T1 = 256: the upper
# bound).  Batches: 2 (one item per workgroup) and 300 (256 workgroups in a one-zone launch: 44 of them take two items)
WINDOWS = (53, 57, 250, 256, 257, 260)
BATCHES = (2, 300)


@functools.lru_cache(maxsize=None)
def _zone16_case(W, B):
    """Parameters, input, upstream gradient and the fp64 results (features, parameter gradients, input gradient)."""
    p = ocnn.init_conv4_params(16, 32, seed=16 + W)
    x = torch.randn(B, 16, W, generator=torch.Generator().manual_seed(W + B))
    w = torch.randn(B, 32, generator=torch.Generator().manual_seed(2))
    pr = {k: v.clone().double().requires_grad_() for k, v in p.items()}
    xr = x.double().requires_grad_()
    yr = ocnn.conv4layers(xr, pr)
    (yr * w.double()).sum().backward()
    return p, x, w, yr.detach(), {k: v.grad for k, v in pr.items()}, xr.grad


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("W", WINDOWS)
def test_zone_of_16_channels_vs_fp64(inn, W, B):
    p, x, w, y_ref, g_ref, dx_ref = _zone16_case(W, B)
    m = inn.Conv4Layers(16, 32).cuda()
    m.load_state_dict(p)
    xc, wc = x.cuda(), w.cuda()
    # fused forward + fused backward
    y = m(xc)
    assert _fwd_path() == FUSED_F32
    (y * wc).sum().backward()
    e = rel_err(y.detach().cpu(), y_ref)
    print(f"W={W} B={B}: features {e:.3g}")
    assert e < TOL
    for k, q in m.named_parameters():
        e = rel_err(q.grad.cpu(), g_ref[k])
        print(f"W={W} B={B}: grad {k} {e:.3g}")
        assert e < TOL, k
    # input gradient: the fused forward, then the layer-wise backward reading GELU'(A4) from the A4 buffer
    m.zero_grad(set_to_none=True)
    xg = xc.clone().requires_grad_()
    yg = m(xg)
    assert _fwd_path() == FUSED_F32
    (yg * wc).sum().backward()
    e = rel_err(xg.grad.cpu(), dx_ref)
    print(f"W={W} B={B}: dx {e:.3g}")
    assert e < TOL
    for k, q in m.named_parameters():
        assert rel_err(q.grad.cpu(), g_ref[k]) < TOL, k
    # inference keeps no activations: the same features, bit for bit
    with torch.no_grad():
        yi = m(xc)
    assert _fwd_path() == FUSED_F32
    assert torch.equal(yi, y.detach())


# ------------------------------------------------------------------ (b) unequal zones, windows, gathered channels
# a made-up montage of 64 electrodes; zones of 16, 13, 12 and 1 channels whose electrodes are neither contiguous nor
# ascending (the chan_idx gather): 13 leaves zero round-up rows under ncg = 4, 12 and 1 run fewer channel groups
MONTAGE = [f"E{i}" for i in range(64)]
_ORDER = [(27 * i + 5) % 64 for i in range(42)]                    # 5, 32, 59, 22, 49, 12, ...: 27 is coprime to 64
ZONES = {"wide": [MONTAGE[i] for i in _ORDER[0:16]], "odd": [MONTAGE[i] for i in _ORDER[16:29]],
         "three": [MONTAGE[i] for i in _ORDER[29:41]], "one": [MONTAGE[i] for i in _ORDER[41:42]]}
ZONE_IDX = ocnn.zone_index_lists(MONTAGE, ZONES)
WL, STEP, T_TRIAL, N_WIN = 250, 125, 512, 3


def test_montage_is_what_the_cases_need():
    assert [len(z) for z in ZONE_IDX] == [16, 13, 12, 1]
    assert len({i for z in ZONE_IDX for i in z}) == 42
    for z in ZONE_IDX[:3]:
        assert z != sorted(z) and any(b != a + 1 for a, b in zip(z, z[1:]))


@functools.lru_cache(maxsize=None)
def _head_state():
    import isd_amd.nn as m
    torch.manual_seed(21)
    return {k: v.detach().clone() for k, v in m.Head("Conv4Layers", MONTAGE, ZONES, 32).state_dict().items()}


def _head(inn, act_dtype="f32"):
    h = inn.Head("Conv4Layers", MONTAGE, ZONES, 32, act_dtype=act_dtype).cuda()
    h.load_state_dict(_head_state())
    return h


@functools.lru_cache(maxsize=None)
def _head_case(B):
    """Input, upstream gradient and the fp64 features / parameter gradients of the head on B trials of 512 samples:
    three windows each.  B = 50: 150 items on 64 workgroups per zone (two or three items each); B = 3: 9 items."""
    x = torch.randn(B, 64, T_TRIAL, generator=torch.Generator().manual_seed(B))
    w = torch.randn(B * N_WIN, 4, 32, generator=torch.Generator().manual_seed(B + 1))
    p = {"head." + k: v.double().requires_grad_() for k, v in _head_state().items()}
    ref = ocnn.forward_head(x.double(), p, list(ZONES), ZONE_IDX, WL, STEP).reshape(B * N_WIN, 4, 32)
    (ref * w.double()).sum().backward()
    return x, w, ref.detach(), {k[len("head."):]: v.grad for k, v in p.items()}


def _run_head(h, x, w, code):
    h.zero_grad(set_to_none=True)
    f = h.forward_windows(x, WL, STEP)
    assert _fwd_path() == code
    (f * w).sum().backward()
    return f.detach(), {k: q.grad.detach().clone() for k, q in h.named_parameters()}


@pytest.mark.parametrize("B", [50, 3])
def test_head_of_unequal_gathered_zones_vs_fp64(inn, B):
    x, w, f_ref, g_ref = _head_case(B)
    h = _head(inn)
    f, g = _run_head(h, x.cuda(), w.cuda(), FUSED_F32)
    assert f.shape == (B * N_WIN, 4, 32)
    for zi, name in enumerate(ZONES):
        e = rel_err(f[:, zi].cpu(), f_ref[:, zi])
        print(f"B={B}: features of zone {name} {e:.3g}")
        assert e < TOL, name
    assert sorted(g) == sorted(g_ref)
    for k in g:
        e = rel_err(g[k].cpu(), g_ref[k])
        print(f"B={B}: grad {k} {e:.3g}")
        assert e < TOL, k
    with torch.no_grad():
        fi = h.forward_windows(x.cuda(), WL, STEP)
    assert _fwd_path() == FUSED_F32
    assert torch.equal(fi, f)


# ------------------------------------------------------------------ (c) repeatability
# Each case runs exactly twice.  The features have no cross-workgroup sums at all; the fused backward leaves its weight
# gradients as per-wave slabs that reduce_jobs_kernel adds in a fixed order (no float atomics), and the chain to cnn1 /
# cnn2 sums inside one workgroup: the parameter gradients repeat bit for bit as well.
def test_zone_of_16_channels_repeats_bit_for_bit(inn):
    p, x, w, _, _, _ = _zone16_case(260, 300)
    m = inn.Conv4Layers(16, 32).cuda()
    m.load_state_dict(p)
    xc, wc = x.cuda(), w.cuda()
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        y = m(xc)
        assert _fwd_path() == FUSED_F32
        (y * wc).sum().backward()
        runs.append((y.detach(), {k: q.grad.detach().clone() for k, q in m.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


def test_head_of_unequal_zones_repeats_bit_for_bit(inn):
    x, w, _, _ = _head_case(50)
    h = _head(inn)
    xc, wc = x.cuda(), w.cuda()
    f0, g0 = _run_head(h, xc, wc, FUSED_F32)
    f1, g1 = _run_head(h, xc, wc, FUSED_F32)
    assert torch.equal(f0, f1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


# ------------------------------------------------------------------ (d) the bf16 twin
@pytest.mark.parametrize("B", [50, 3])
def test_bf16_head_of_unequal_gathered_zones(inn, B):
    """The same head with bf16 activations (conv4_fused_fwd_bf16_kernel / conv4_fused_bwd_bf16_kernel).  Stated
    tolerances of test_bf16_fused_raw_eeg_head_vs_fp32: features 8e-3 and parameter gradients 2e-2 of the tensor's
    largest magnitude against the fp32 kernels on the same parameters; features 8e-3 against the fp64 oracle."""
    x, w, f_ref, _ = _head_case(B)
    xc, wc = x.cuda(), w.cuda()
    f32, g32 = _run_head(_head(inn), xc, wc, FUSED_F32)
    f16, g16 = _run_head(_head(inn, "bf16"), xc, wc, FUSED_BF16)
    e = rel_err(f16.cpu(), f32.cpu())
    print(f"B={B}: bf16 features vs fp32 {e:.3g}")
    assert 0 < e < 8e-3
    for k in g32:
        e = rel_err(g16[k].cpu(), g32[k].cpu())
        print(f"B={B}: bf16 grad {k} vs fp32 {e:.3g}")
        assert e < 2e-2, k
    e = rel_err(f16.cpu(), f_ref)
    print(f"B={B}: bf16 features vs fp64 {e:.3g}")
    assert e < 8e-3
