"""GPU: training RecNeXt-T / S / B.  The wide linear-attention core (rcx_linear_attention_wide_fwd / _bwd) against float64 autograd of
tests/ls_eager.py's _attend; every block shape of the T / S / B table in train mode against the operator chain and against the reference's
float64 fixtures (tests/golden/ls_grad_*.npz); whole models (loss, every gradient, an AdamW step, then inference); bf16 autocast; the launch
path; frozen-BatchNorm fine-tuning."""
import copy

import pytest
import torch
import torch.nn.functional as F

from recnext_amd import lsmodels, ops
from tests.ls_eager import _attend, eager_token_mixer, token_half
from tests.test_ls_train_cpu import GRAD_NAMES, build_train_block, load_grad_case

DEV = torch.device("cuda:0")
TOL = {torch.float32: 2e-4, torch.bfloat16: 2e-2, torch.float16: 4e-3}
# the T / S / B table at 224 x 224: (name, C, stage, plane, constructor heads, mlp ratio)
TABLE = [("b_s0", 128, 0, 28, 1, 2), ("t_s1", 128, 1, 14, 1, 2), ("sb_s1", 256, 1, 14, 1, 2), ("t_s2", 256, 2, 7, 1, 2), ("sb_s2", 384, 2, 7, 1, 2),
         ("all_s3", 512, 3, 4, 2, 1.5)]
PLANES = {16: (4, 4), 45: (5, 9), 49: (7, 7), 196: (14, 14), 576: (24, 24)}


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _wide_ref(qpre, kpre, v, pe, heads):
    """float64 restatement: qpre, kpre (b, n, cqk), v, pe (b, n, cv) -> (b, n, cv), through tests/ls_eager.py's _attend."""
    b, n, cqk = qpre.shape
    cv = v.shape[2]
    hd = lambda t, d: t.view(b, n, heads, d).permute(0, 2, 3, 1)                     # (b, heads, d, n)
    q, k = hd(F.elu(qpre) + 1.0, cqk // heads), hd(F.elu(kpre) + 1.0, cqk // heads)
    o = _attend(q, k, hd(v, cv // heads), n ** -0.5)                                    # (b, heads, n, dv)
    return o.permute(0, 2, 1, 3).reshape(b, n, cv) + pe


def _core_inputs(b, n, cqk, cv, dtype, seed):
    h, w = PLANES[n]
    g = torch.Generator(device=DEV).manual_seed(seed)
    mk = lambda *s: (torch.randn(*s, device=DEV, generator=g) * 0.7).to(dtype)
    qpre, kpre = mk(b, n, cqk), mk(b, n, cqk)
    v = mk(b, cv, h, w).contiguous(memory_format=torch.channels_last)
    pe = mk(b, cv, h, w).contiguous(memory_format=torch.channels_last)
    gout = mk(b, cv, h, w).contiguous(memory_format=torch.channels_last)
    return qpre, kpre, v, pe, gout


def _run_core(fn, qpre, kpre, v, pe, gout, heads):
    ins = [t.clone().requires_grad_(True) for t in (qpre, kpre, v, pe)]
    out = fn.apply(*ins, heads)
    out.backward(gout)
    return out.detach(), [t.grad for t in ins]


tokv = lambda t: t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("n", [16, 45, 49, 196, 576])
@pytest.mark.parametrize("dk,dv", [(96, 96), (64, 128), (32, 64), (128, 64), (64, 64)])
def test_wide_core_against_float64(dk, dv, n, heads, dtype):
    b = 2
    cqk, cv = dk * heads, dv * heads
    qpre, kpre, v, pe, gout = _core_inputs(b, n, cqk, cv, dtype, seed=dk * 1000 + dv * 10 + n + heads)
    ref_in = [t.double().clone().requires_grad_(True) for t in (qpre, kpre, tokv(v), tokv(pe))]
    ref = _wide_ref(*ref_in, heads)
    ref.backward(tokv(gout).double())
    out, grads = _run_core(ops.LinearAttentionWideCoreFn, qpre, kpre, v, pe, gout, heads)
    tol = TOL[dtype]
    assert out.dtype == dtype and out.is_contiguous(memory_format=torch.channels_last)
    assert _rel(tokv(out), ref) < tol
    for name, g, r in zip(("qpre", "kpre", "v", "pe"), [grads[0], grads[1], tokv(grads[2]), tokv(grads[3])], ref_in):
        assert g.dtype == dtype, name
        assert _rel(g, r.grad) < tol, name
    # bitwise deterministic, and an image's results do not depend on the batch
    out2, grads2 = _run_core(ops.LinearAttentionWideCoreFn, qpre, kpre, v, pe, gout, heads)
    assert torch.equal(out2, out) and all(torch.equal(a, c) for a, c in zip(grads2, grads))
    one = [t[1:2].contiguous() for t in (qpre, kpre)] + [t[1:2].contiguous(memory_format=torch.channels_last) for t in (v, pe, gout)]
    out1, grads1 = _run_core(ops.LinearAttentionWideCoreFn, *one, heads)
    assert torch.equal(out1, out[1:2]) and all(torch.equal(a, c[1:2]) for a, c in zip(grads1, grads))
    if dk == dv == 64:                           # the existing core takes this head too: the two agree within the same bars
        outc, gradsc = _run_core(ops.LinearAttentionCoreFn, qpre, kpre, v, pe, gout, heads)
        assert _rel(out, outc) < tol
        for a, c in zip(grads, gradsc):
            assert _rel(a, c) < tol


@pytest.mark.gpu
def test_wide_core_argument_checks_raise_value_error():
    qpre, kpre, v, pe, gout = _core_inputs(2, 16, 64, 128, torch.float32, seed=3)
    bad = [
        (qpre.cpu(), kpre, v, pe, 1),                               # device
        (qpre, kpre[:, :, :32].contiguous(), v, pe, 1),             # kpre's width differs from qpre's
        (qpre, kpre, v, pe[:, :64], 1),                             # pe's shape
        (qpre, kpre, v, pe.bfloat16(), 1),                          # pe's dtype
        (qpre.bfloat16(), kpre.bfloat16(), v, pe, 1),               # q / k dtype differs from v's
        (qpre, kpre, v, pe, 3),                                     # heads do not divide the channels
        (qpre[:, :8].contiguous(), kpre[:, :8].contiguous(), v, pe, 1),     # token count
        (torch.randn(2, 16, 264, device=DEV), torch.randn(2, 16, 264, device=DEV), v, pe, 1),   # Dk 264 > 128
        (qpre.double(), kpre.double(), v.double(), pe.double(), 1),  # dtype
    ]
    for args in bad:
        with pytest.raises(ValueError):
            ops.linear_attention_wide(*args)
    with pytest.raises(ValueError):
        ops.linear_attention_wide_backward(qpre, kpre, v, gout[:, :64], 1)
    with pytest.raises(ValueError):
        ops.linear_attention_wide_backward(qpre, kpre, v.cpu(), gout, 1)


def _randomize_bn(module, seed):
    g = torch.Generator().manual_seed(seed)
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.3)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 0.8 + 0.4)
            m.weight.data.copy_(torch.rand(m.weight.shape, generator=g) * 0.8 + 0.6)
            m.bias.data.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)


def _block_pair(c, stage, heads, ratio, seed):
    torch.manual_seed(seed)
    ref = lsmodels.MetaNeXtBlock(c, ratio, num_heads=heads, stage=stage, token_mixer=eager_token_mixer)
    _randomize_bn(ref, seed)
    hip = lsmodels.MetaNeXtBlock(c, ratio, num_heads=heads, stage=stage)
    hip.load_state_dict(ref.state_dict(), strict=True)
    return ref.to(DEV), hip.to(DEV)


def _token_half_step(blk, x, gy, eager):
    x = x.clone().requires_grad_(True)
    r, t = token_half(blk, x) if eager else blk.token_half(x)
    (t * gy).sum().backward()
    return r.detach(), t.detach(), x.grad


def _check_block(ref, hip, r_ref, t_ref, gx_ref, r, t, gx):
    assert _rel(t, t_ref) < 1e-4 and _rel(r, r_ref) < 1e-4
    assert t.is_contiguous(memory_format=torch.channels_last)
    assert _rel(gx, gx_ref) < 2e-3
    pr = {k: p for k, p in ref.named_parameters() if not k.startswith("channel_mixer.")}
    po = dict(hip.named_parameters())
    scale = max(float(p.grad.abs().max()) for p in pr.values() if p.grad is not None)
    for k, p in pr.items():
        if p.grad is None:
            assert po[k].grad is None, k
            continue
        assert po[k].grad is not None, k
        assert float((po[k].grad - p.grad).abs().max()) < 2e-3 * float(p.grad.abs().max()) + 1e-5 * scale, k
    for (k, br), (_, bo) in zip(ref.named_buffers(), hip.named_buffers()):
        assert torch.allclose(br.float(), bo.float(), atol=1e-5, rtol=1e-4), k


@pytest.mark.gpu
@pytest.mark.parametrize("case", TABLE, ids=[c[0] for c in TABLE])
def test_block_training_matches_eager(case):
    """Train mode, batch statistics: the HIP token half against the operator chain with the same state_dict (randomised BatchNorms)."""
    _, c, stage, h, heads, ratio = case
    ref, hip = _block_pair(c, stage, heads, ratio, seed=c + stage)
    ref.train(), hip.train()
    g = torch.Generator(device=DEV).manual_seed(c)
    x = torch.randn(2, c, h, h, device=DEV, generator=g).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(2, c, h, h, device=DEV, generator=g)
    _check_block(ref, hip, *_token_half_step(ref, x, gy, True), *_token_half_step(hip, x, gy, False))


@pytest.mark.gpu
@pytest.mark.parametrize("name", GRAD_NAMES)
def test_block_training_matches_reference_fixture(name):
    """The HIP training step against the reference's float64 step: within the bars above, or within 3x the float32 operator chain's own distance
    from the fixture (float32 batch statistics of a small batch are themselves ~1e-4 away from float64)."""
    x, gy, sd, t_ref, gx_ref, grads, running, meta = load_grad_case(name)

    def run(token_mixer):
        blk = build_train_block(meta, sd, token_mixer=token_mixer).to(DEV)
        xx = x.float().to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        _, t = token_half(blk, xx) if token_mixer else blk.token_half(xx)
        (t * gy.float().to(DEV)).sum().backward()
        params = dict(blk.named_parameters())
        return t.detach().cpu(), xx.grad.cpu(), {k: params[k].grad.cpu() for k in grads}, blk.state_dict()

    hip, eag = run(None), run(eager_token_mixer)
    dist = lambda got, want: float((got.double() - want).abs().max())
    assert dist(hip[0], t_ref) <= max(1e-4 * float(t_ref.abs().max()), 3 * dist(eag[0], t_ref))
    assert dist(hip[1], gx_ref) <= max(2e-3 * float(gx_ref.abs().max()), 3 * dist(eag[1], gx_ref))
    scale = max(float(v.abs().max()) for v in grads.values())
    for k, gr in grads.items():
        assert dist(hip[2][k], gr) <= max(2e-3 * float(gr.abs().max()) + 1e-5 * scale, 3 * dist(eag[2][k], gr)), k
    for k, v in running.items():
        assert torch.allclose(hip[3][k].cpu().double(), v, atol=1e-5, rtol=1e-4), k


@pytest.mark.gpu
@pytest.mark.parametrize("case", [TABLE[1], TABLE[4], TABLE[5]], ids=["t_s1", "sb_s2", "all_s3"])
def test_frozen_bn_fine_tuning_matches_eager(case):
    """eval() with parameters that require grad (frozen BatchNorm statistics): the training form, with running statistics, gives eager's gradients."""
    _, c, stage, h, heads, ratio = case
    ref, hip = _block_pair(c, stage, heads, ratio, seed=7 * c + stage)
    ref.eval(), hip.eval()
    g = torch.Generator(device=DEV).manual_seed(c + 1)
    x = torch.randn(2, c, h, h, device=DEV, generator=g).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(2, c, h, h, device=DEV, generator=g)
    _check_block(ref, hip, *_token_half_step(ref, x, gy, True), *_token_half_step(hip, x, gy, False))


def _model_pair(name):
    torch.manual_seed(0)
    ref = lsmodels.create_model(name, token_mixer=eager_token_mixer, drop_path_rate=0.0)
    _randomize_bn(ref, 11)
    hip = lsmodels.create_model(name, drop_path_rate=0.0)
    hip.load_state_dict(ref.state_dict(), strict=True)
    return ref.to(DEV).train(), hip.to(DEV).to(memory_format=torch.channels_last).train()


def _loss(net, x, y):
    return F.cross_entropy(net(x), y)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["recnext_t", "recnext_s", "recnext_b"])
def test_whole_model_training_step_matches_eager(name):
    """f32 HIP against the f32 operator chain, each measured from the chain in float64: through 20-30 train-mode BatchNorms of small batches (stage 3:
    16 samples a channel an image) the f32 chain's own gradients are up to ~4 % (max-norm) from float64 at batch 2, so every parameter's gradient is compared in
    L2 norm, the HIP step within 5x the f32 chain's distance or 5 % (a wrong gradient anywhere is off by O(1)); the whole gradient vector and
    the loss within 4x the f32 chain's distance (the library's own convs pick their algorithms per run, so the f32 chain's distance varies)."""
    ref, hip = _model_pair(name)
    ref64 = copy.deepcopy(ref).double()
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(4, 3, 224, 224, device=DEV, generator=g)
    y = torch.randint(0, 1000, (4,), device=DEV, generator=g)
    l64, lr, lh = _loss(ref64, x.double(), y), _loss(ref, x, y), _loss(hip, x.contiguous(memory_format=torch.channels_last), y)
    for loss in (l64, lr, lh):
        loss.backward()
    dist = lambda a, b: float((a.detach().double() - b.detach().double()).abs().max())
    assert dist(lh.detach(), l64) <= max(1e-4 * abs(float(l64)), 4 * dist(lr, l64))
    ph, pr = dict(hip.named_parameters()), dict(ref.named_parameters())
    # a gradient that is zero in exact arithmetic (a conv bias or the depthwise 1x1 `sk` scale in front of a train-mode BatchNorm: the batch
    # statistics remove them) is rounding noise on every side: the floor is 1e-2 of the model's RMS gradient
    err = lambda a, b: float((a.detach().double() - b.detach().double()).norm())
    allg = torch.cat([p.grad.flatten() for p in ref64.parameters()])
    rms = float(allg.norm()) / allg.numel() ** 0.5
    for k, p in ref64.named_parameters():
        assert ph[k].grad is not None, k
        bar = max(5e-2 * float(p.grad.norm()), 5 * err(pr[k].grad, p.grad), 1e-2 * rms * p.numel() ** 0.5)
        assert err(ph[k].grad, p.grad) <= bar, (k, err(ph[k].grad, p.grad), err(pr[k].grad, p.grad), float(p.grad.norm()), rms * p.numel() ** 0.5)
    assert err(torch.cat([ph[k].grad.flatten() for k, _ in ref64.named_parameters()]), allg) <= max(2e-3 * float(allg.norm()),
                                                                                                  4 * err(torch.cat([p.grad.flatten() for p in ref.parameters()]), allg))
    l2 = lambda a, b: err(a, b) / (float(b.detach().double().norm()) + 1e-30)
    # one AdamW step on each, then inference: the packs must pick up the new weights and running statistics
    for net in (ref64, ref, hip):
        torch.optim.AdamW(net.parameters(), lr=1e-3).step()
        net.eval()
    with torch.no_grad():
        a64, a = ref64(x.double()), ref(x)
        b = hip(x.contiguous(memory_format=torch.channels_last))
    assert l2(b, a64) <= max(1e-3, 4 * l2(a, a64))


@pytest.mark.gpu
def test_bf16_autocast_step():
    ref, hip = _model_pair("recnext_s")
    g = torch.Generator(device=DEV).manual_seed(6)
    x = torch.randn(4, 3, 224, 224, device=DEV, generator=g)
    y = torch.randint(0, 1000, (4,), device=DEV, generator=g)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lr = _loss(ref, x, y)
        lh = _loss(hip, x.contiguous(memory_format=torch.channels_last), y)
    lr.backward(), lh.backward()
    assert abs(float(lh) - float(lr)) < 5e-2 * max(1.0, abs(float(lr)))
    ph = dict(hip.named_parameters())
    for k, p in ref.named_parameters():
        assert ph[k].grad is not None and bool(torch.isfinite(ph[k].grad).all()), k
    gr = torch.cat([p.grad.flatten() for p in ref.parameters()])
    gh = torch.cat([ph[k].grad.flatten() for k, _ in ref.named_parameters()])
    assert float(F.cosine_similarity(gr.double(), gh.double(), dim=0)) > 0.95


@pytest.mark.gpu
def test_bf16_module_training_step():
    """A bf16 module trains (the A family's handling: the cores take the activations' type, gradients in the parameters' type)."""
    _, c, stage, h, heads, ratio = TABLE[5]
    _, hip = _block_pair(c, stage, heads, ratio, seed=3)
    hip = hip.bfloat16().train()
    x = torch.randn(2, c, h, h, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    _, t = hip.token_half(x)
    t.float().sum().backward()
    assert t.dtype == torch.bfloat16 and bool(torch.isfinite(x.grad.float()).all())
    for k, p in hip.named_parameters():
        if not k.startswith("channel_mixer."):
            assert p.grad is not None and p.grad.dtype == torch.bfloat16 and bool(torch.isfinite(p.grad.float()).all()), k


@pytest.mark.gpu
def test_launch_path_reaches_the_wide_core(monkeypatch):
    calls = {k: 0 for k in ("linear_attention_wide", "linear_attention_wide_backward", "linear_attention_core", "linear_attention_core_backward")}
    for k in calls:
        real = getattr(ops, k)
        monkeypatch.setattr(ops, k, lambda *a, _k=k, _f=real, **kw: (calls.__setitem__(_k, calls[_k] + 1), _f(*a, **kw))[1])

    def step(case):
        _, c, stage, h, heads, ratio = case
        _, hip = _block_pair(c, stage, heads, ratio, seed=1)
        x = torch.randn(2, c, h, h, device=DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        hip.train().token_half(x)[1].sum().backward()
        out = dict(calls)
        for k in calls:
            calls[k] = 0
        return out

    want_wide = {"linear_attention_wide": 1, "linear_attention_wide_backward": 1, "linear_attention_core": 0, "linear_attention_core_backward": 0}
    assert step(TABLE[4]) == want_wide                                   # S stage 2: 96-wide heads
    assert step(TABLE[5]) == want_wide                                   # stage 3: LinearAttention3, (64, 128)
    assert step(TABLE[1]) == {"linear_attention_wide": 0, "linear_attention_wide_backward": 0, "linear_attention_core": 1,
                              "linear_attention_core_backward": 1}      # T stage 1: 32-wide heads stay on the existing core
