"""GPU parity of the BatchNorm heads of the reference's head registry -- CVBlock (fast.py:32-100) and
HeadConv_Paper_Version (fast.py:170-196) -- against golden vectors captured from the reference and the oracle."""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from oracle import cnn as ocnn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inn():
    import isd_amd.nn as m
    assert torch.cuda.is_available()
    return m


def _sd(g, prefix):
    return {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}


def _check_against_golden(m, g, tag, grad_tol=1e-4, cancel=()):
    """``cancel``: parameters whose gradient vanishes analytically (BN gamma/beta directly followed by another
    BatchNorm); the reference's own values are fp32 cancellation residue, so they are compared on the gradient scale."""
    m.load_state_dict(_sd(g, f"{tag}.sd."))
    x = torch.from_numpy(g[f"{tag}.x"]).cuda()
    m.eval()
    with torch.no_grad():
        y_eval = m(x)
    assert y_eval.shape == (x.shape[0], 32)
    assert rel_err(y_eval.cpu(), g[f"{tag}.y_eval"]) < 1e-4
    m.train()
    y = m(x)
    assert rel_err(y.detach().cpu(), g[f"{tag}.y_train"]) < 1e-4
    y.square().sum().backward()
    scale = max(float(np.abs(g[k]).max()) for k in g.files if k.startswith(f"{tag}.grad."))
    for k, p in m.named_parameters():
        want = g[f"{tag}.grad.{k}"]
        tol = grad_tol * max(float(np.abs(want).max()), (5e-2 if k.startswith(cancel) else 1e-3) * scale)
        assert np.abs(p.grad.cpu().numpy() - want).max() < tol + 1e-7, k
    sd_after = _sd(g, f"{tag}.sd_after.")
    for k, v in m.state_dict().items():
        if "running" in k:
            assert rel_err(v.cpu(), sd_after[k]) < 1e-4, k
        if "num_batches_tracked" in k:
            assert int(v) == int(sd_after[k])


@pytest.mark.parametrize("tag,C", [("z6", 6), ("z15", 15)])
def test_cvblock_matches_reference_golden(inn, tag, C):
    _check_against_golden(inn.CVBlock(C, 32, dropout=0.0).cuda(), load_golden("g10_cvblock.npz"), tag, cancel=("bn1.",))


def _vs_oracle(m, fn, x, F, bn_floor_prefix=()):
    p = {k: v.detach().cpu().clone().double() for k, v in m.state_dict().items()}
    for k, v in p.items():
        if "running" not in k and "num_batches" not in k:
            v.requires_grad_()
    w = torch.randn(x.shape[0], F)
    m.train()
    y = m(x.cuda())
    (y * w.cuda()).sum().backward()
    yr = fn(x.double(), p, training=True)
    (yr * w.double()).sum().backward()
    assert rel_err(y.detach().cpu(), yr.detach()) < 1e-4
    scale = max(float(v.grad.abs().max()) for v in p.values() if v.grad is not None)
    for k, q in m.named_parameters():
        want = p[k].grad
        floor = 5e-2 if k.startswith(bn_floor_prefix) else 1e-3
        tol = 1e-4 * max(float(want.abs().max()), floor * scale)
        assert float((q.grad.cpu().double() - want).abs().max()) < tol + 1e-7, k
    for k, v in m.state_dict().items():
        if "running" in k:
            assert rel_err(v.cpu(), p[k]) < 1e-4, k


@pytest.mark.parametrize("C,B,F", [(4, 3, 16), (10, 70, 32), (64, 4, 8)])
def test_cvblock_vs_oracle(inn, C, B, F):
    torch.manual_seed(C)
    m = inn.CVBlock(C, F, dropout=0.0).cuda()
    with torch.no_grad():
        for bn in m._bns():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.3, 0.3)
    _vs_oracle(m, ocnn.cvblock, torch.randn(B, C, 250), F, bn_floor_prefix=("bn1.",))


def test_cvblock_contract(inn):
    m = inn.CVBlock(6, 32).cuda().eval()
    x = torch.randn(3, 6, 250, device="cuda")
    with torch.no_grad():
        assert torch.equal(m(x), m(x.unsqueeze(1)))                 # 4-D input accepted (fast.py:79-80)
        with pytest.raises(RuntimeError):
            m(torch.randn(3, 6, 500, device="cuda"))                # projector width is tied to 250 samples
    assert m.flat_dim == 256 and m.projector.weight.shape == (32, 256)
    m.train()
    m.p = 0.0
    ref = m(x).detach()
    m.p = 0.5
    a, b = m(x).detach(), m(x).detach()
    assert not torch.equal(a, b) and not torch.equal(a, ref)        # train-mode dropout draws a fresh mask per call


@pytest.mark.parametrize("tag,C", [("z6", 6), ("z15", 15)])
def test_paperhead_matches_reference_golden(inn, tag, C):
    # the conv bias in front of BatchNorm has an analytically zero gradient (rounding residue in the reference)
    _check_against_golden(inn.HeadConv_Paper_Version(C, 32).cuda(), load_golden("g11_paperhead.npz"), tag,
                          cancel=("cnn1_t.bias",))


@pytest.mark.parametrize("C,T,B,F", [(4, 250, 3, 32), (10, 125, 70, 16), (64, 250, 4, 48), (20, 46, 5, 9)])
def test_paperhead_vs_oracle(inn, C, T, B, F):
    torch.manual_seed(C + T)
    m = inn.HeadConv_Paper_Version(C, F).cuda()
    with torch.no_grad():
        for bn in m._bns():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.3, 0.3)
    _vs_oracle(m, ocnn.headconv_paper, torch.randn(B, C, T), F, bn_floor_prefix=("cnn1_t.bias",))
    with pytest.raises(Exception):
        inn.HeadConv_Paper_Version(C, F).cuda()(torch.randn(2, C, 40, device="cuda"))    # too short for four stages


@pytest.mark.parametrize("head,enc", [("HeadConv_Paper_Version", "headconv_paper"), ("CVBlock", "cvblock"),
                                      ("EEGNet_Encoder", "eegnet_encoder")])
def test_fast_with_registry_heads_vs_oracle(inn, head, enc):
    """The head registry of fast.py:203: FAST(config.head=<name>) in the trained mode, forward + every gradient."""
    electrodes = ["Fp1", "Fp2", "F3", "F4", "C3", "C4", "O1", "O2", "Pz"]
    zones = {"Frontal": ["Fp1", "Fp2", "F3", "F4"], "Central": ["C4", "C3", "Pz"], "Occipital": ["O2", "O1"]}
    cfg = inn.fast_config(electrodes, zones, dim_cnn=16, dim_token=16, seq_len=500, n_classes=3, num_layers=1,
                          num_heads=4, dropout=0.0, head=head)
    torch.manual_seed(3)
    m = inn.FAST(cfg).cuda()
    for e in m.head.encoders.values():
        if hasattr(e, "p"):
            e.p = 0.0                                               # the oracle has no dropout stream
    p = {k: v.detach().cpu().clone().double() for k, v in m.state_dict().items()}
    for k, v in p.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_()
    x = torch.randn(6, len(electrodes), 500)
    names = list(zones)
    idx = [[electrodes.index(c) for c in zones[z]] for z in names]
    m.train()
    lg = m(x.cuda())
    lg.square().sum().backward()
    ref = ocnn.default_logits(x.double(), p, names, idx, 4, 1, encoder=getattr(ocnn, enc), training=True)
    ref.square().sum().backward()
    assert lg.shape == (6, 3) and rel_err(lg.detach().cpu(), ref.detach()) < 1e-4
    scale = max(float(v.grad.abs().max()) for v in p.values() if v.grad is not None)
    for k, q in m.named_parameters():
        want = p[k].grad
        tol = 2e-4 * max(float(want.abs().max()), 5e-2 * scale)
        assert float((q.grad.cpu().double() - want).abs().max()) < tol + 1e-7, k
    # input attributions: the eval-mode network differentiated w.r.t. the trials, end to end (zones own their channels,
    # overlapping windows add, BatchNorm on its running statistics)
    m.eval()
    xg = x.cuda().requires_grad_()
    m(xg)[:, 1].sum().backward()
    p2 = {k: v.detach().cpu().clone().double() for k, v in m.state_dict().items()}
    xr = x.double().requires_grad_()
    ocnn.default_logits(xr, p2, names, idx, 4, 1, encoder=getattr(ocnn, enc), training=False)[:, 1].sum().backward()
    assert rel_err(xg.grad.cpu(), xr.grad) < 2e-4
    with pytest.raises(KeyError):
        inn.FAST(inn.fast_config(electrodes, zones, head="NoSuchHead"))


@pytest.mark.parametrize("head", ["EEGNet_Encoder", "CVBlock", "HeadConv_Paper_Version"])
def test_zone_batched_launches_equal_per_zone_calls(inn, head, monkeypatch):
    """Head(...) with one BatchNorm encoder per zone (fast.py:203-210): the zone-batched launches (isd_zone_batch_*:
    launch i of all eight zones as one kernel) give the per-zone calls' outputs bit for bit, their running statistics
    and -- up to the order of the fp32 / fp64 atomic sums -- their parameter gradients, in train mode (with dropout:
    the masks are counter-based per zone) and in eval mode; an input that needs a gradient keeps the per-zone path."""
    import isd_amd._lib as L

    def run(off, train, p=None):
        if off:
            monkeypatch.setenv("ISD_ZONE_BATCH_OFF", "1")
        else:
            monkeypatch.delenv("ISD_ZONE_BATCH_OFF", raising=False)
        torch.manual_seed(5)
        h = inn.Head(head, ocnn.ELECTRODES, ocnn.ZONES, 32).cuda().train(train)
        ids = []
        for e in h.encoders.values():
            if p is not None and hasattr(e, "p"):
                e.p = p
            if hasattr(e, "_stream_id"):
                ids.append(e._stream_id)
        x = torch.randn(21, 64, 250, device="cuda")
        w = torch.randn(21, 8, 32, device="cuda")
        if train:
            f = h(x)
            (f * w).sum().backward()
            g = torch.cat([q.grad.reshape(-1) for q in h.parameters()])
        else:
            with torch.no_grad():
                f = h(x)
            g = None
        return h, ids, f.detach(), g, torch.cat([b.reshape(-1).float() for b in h.buffers()])

    h0, ids0, f0, g0, b0 = run(True, True, p=0.0)
    h1, ids1, f1, g1, b1 = run(False, True, p=0.0)
    assert torch.equal(f0, f1)
    assert float((g0 - g1).abs().max() / g0.abs().max()) < 1e-5
    assert float((b0 - b1).abs().max()) < 1e-6
    # dropout on: same masks when the encoders' dropout streams are the same
    if ids0:
        def with_streams(off):
            if off:
                monkeypatch.setenv("ISD_ZONE_BATCH_OFF", "1")
            else:
                monkeypatch.delenv("ISD_ZONE_BATCH_OFF", raising=False)
            torch.manual_seed(6)
            h = inn.Head(head, ocnn.ELECTRODES, ocnn.ZONES, 32).cuda().train()
            for e, sid in zip(h.encoders.values(), ids0):
                e._stream_id = sid
            x = torch.randn(9, 64, 250, device="cuda")
            return h(x).detach()
        assert torch.equal(with_streams(True), with_streams(False))
    # eval mode, no gradients
    _, _, e0, _, _ = run(True, False)
    _, _, e1, _, _ = run(False, False)
    assert torch.equal(e0, e1)
    # an input gradient: per-zone path, still correct
    monkeypatch.delenv("ISD_ZONE_BATCH_OFF", raising=False)
    x = torch.randn(5, 64, 250, device="cuda", requires_grad=True)
    assert not h1._zone_batchable(list(h1.encoders.values()), x)
    h1(x).sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    # the recorder's own errors
    lib = L.lib()
    with pytest.raises(L.IsdError):
        L.check(lib.isd_zone_batch_launch(0))                          # nothing open
    L.check(lib.isd_zone_batch_begin())
    with pytest.raises(L.IsdError):
        L.check(lib.isd_zone_batch_begin())                            # already open
    L.check(lib.isd_zone_batch_abort())
    L.check(lib.isd_zone_batch_begin())
    L.check(lib.isd_zone_batch_launch(0))                              # an empty batch launches nothing


def test_zones_on_both_sides_of_128_channels_take_the_per_zone_path(inn):
    """a head whose zones straddle 128 channels records different kernel chains (the spatial projection
    takes whole rows per workgroup from 128 channels on), so it must not be zone-batched -- it falls back to the
    per-zone streams and matches the oracle zone by zone."""
    electrodes = [f"E{i}" for i in range(140)]
    zones = {"Wide": electrodes[:130], "Narrow": electrodes[130:]}
    torch.manual_seed(2)
    h = inn.Head("EEGNet_Encoder", electrodes, zones, 16).cuda().eval()
    x = torch.randn(3, 140, 250, device="cuda")
    assert not h._zone_batchable(list(h.encoders.values()), x)
    with torch.no_grad():
        f = h(x)
    assert f.shape == (3, 2, 16)
    for zi, (area, enc) in enumerate(h.encoders.items()):
        p = {k: v.detach().cpu().double() for k, v in enc.state_dict().items()}
        idx = torch.tensor([electrodes.index(e) for e in zones[area]])
        ref = ocnn.eegnet_encoder(x.cpu().double()[:, idx], p, training=False)
        assert rel_err(f[:, zi].cpu(), ref) < 1e-4, area


@pytest.mark.parametrize("head", ["EEGNet_Encoder", "CVBlock", "HeadConv_Paper_Version"])
def test_batchnorm_heads_are_bitwise_repeatable(inn, head):
    """VERDICT r2 (missing 2): the reference trains with cudnn.deterministic (src/fast/utils.py:104-114).  The batch
    sums of these heads (BatchNorm statistics, BatchNorm backward sums, the stage-1 correlation sums) come from
    thousands of workgroups; they are accumulated exactly with integer atomics (csrc/exact.h), so outputs, every
    gradient and the running statistics carry the same bits on every run -- under a different launch interleaving too
    (other work on a second stream) -- and a 20-step AdamW run ends on identical parameters."""
    def run(disturb):
        torch.manual_seed(9)
        h = inn.Head(head, ocnn.ELECTRODES, ocnn.ZONES, 32).cuda().train()
        for zi, e in enumerate(h.encoders.values()):
            if hasattr(e, "p"):
                e.p = 0.25
                e._stream_id = 3 + zi
                e._calls = 0
        gen = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(37, 64, 250, device="cuda", generator=gen)
        w = torch.randn(37, 8, 32, device="cuda", generator=gen)
        side = torch.cuda.Stream()
        junk = torch.randn(2048, 2048, device="cuda", generator=gen)
        opt = torch.optim.AdamW(h.parameters(), lr=5e-3)
        outs = []
        for step in range(20):
            if disturb:
                with torch.cuda.stream(side):                       # competes for the CUs: workgroups arrive in another order
                    for _ in range(3):
                        junk = junk @ junk * 1e-3
            opt.zero_grad(set_to_none=True)
            f = h(x)
            (f * w).sum().backward()
            if step == 0:
                outs.append(f.detach().clone())
                outs.append(torch.cat([q.grad.reshape(-1) for q in h.parameters()]).clone())
            opt.step()
        torch.cuda.synchronize()
        outs.append(torch.cat([q.detach().reshape(-1) for q in h.parameters()]).clone())
        outs.append(torch.cat([b.detach().reshape(-1).float() for b in h.buffers()]).clone())
        return outs
    a, b, c = run(False), run(False), run(True)
    for name, ta, tb, tc in zip(("output", "gradient", "parameters after 20 steps", "buffers"), a, b, c):
        assert torch.equal(ta, tb), (head, name, "same launch pattern")
        assert torch.equal(ta, tc), (head, name, "disturbed launch pattern")
    assert bool(torch.isfinite(a[2]).all())


def test_paperhead_ignores_the_dropout_seed_counter(inn):
    """``isd_amd.graph`` hands every encoder that has ``set_seed_counter`` the device-resident dropout step counter,
    whenever the capture happens.  HeadConv_Paper_Version draws no masks: with a plan already cached (a forward has
    run) setting and clearing the counter is a no-op, and the next forward carries the bits of a fresh module with the
    same parameters."""
    torch.manual_seed(11)
    m = inn.HeadConv_Paper_Version(6, 32).cuda().eval()
    x = torch.randn(5, 6, 250, device="cuda")
    with torch.no_grad():
        m(x)
        m.set_seed_counter(torch.zeros(1, dtype=torch.int64, device="cuda"))
        m.set_seed_counter(None)
        y = m(x)
        fresh = inn.HeadConv_Paper_Version(6, 32).cuda().eval()
        fresh.load_state_dict(m.state_dict())
        assert torch.equal(y, fresh(x))
    assert not hasattr(m, "_stream_id")
