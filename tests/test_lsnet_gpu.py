"""GPU: the HIP token half of the LSNet-style RecNeXt-T / S / B (rcx_ls_recattn_fwd / rcx_ls_la3_fwd) against the reference's fixtures and the
operator restatement tests/ls_eager.py; numerics in three dtypes, folding, determinism, argument checks, the launch path and whole models."""
import copy

import pytest
import torch

from recnext_amd import lsmodels, models, ops
from recnext_amd.graph import GraphedInference
from tests.ls_eager import eager_token_mixer, token_half
from tests.test_lsnet_cpu import NAMES, block_cases, build_block, load_block

DEV = torch.device("cuda:0")


def cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def hip_block(name):
    x, r, t_s, sd, meta = load_block(name)
    return build_block(meta, sd).to(DEV), x, r, t_s, sd, meta


def bf16_bar(got, want):
    return bool(((got.float().cpu() - want).abs() <= 1e-2 + 1e-2 * want.abs()).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", block_cases())
def test_token_half_matches_the_fixture(name):
    blk, x, r, t_s, sd, meta = hip_block(name)
    s = meta["split"]
    with torch.no_grad():
        got_r, got_t = blk.token_half(cl(x))
        assert float((got_r.cpu() - r).abs().max()) <= 2e-4
        assert float((got_t[:, :s].cpu() - t_s).abs().max()) <= 2e-4
        assert torch.equal(got_t[:, s:], got_r[:, s:])
        for dt in (torch.bfloat16, torch.float16):               # x is bf16-representable: the fixture is the float32 result on rounded input
            br, bt = blk.token_half(cl(x).to(dt))
            assert br.dtype == dt and bt.dtype == dt
            assert bf16_bar(br, r) and bf16_bar(bt[:, :s], t_s), dt
            assert torch.equal(bt[:, s:], br[:, s:])


@pytest.mark.gpu
@pytest.mark.parametrize("name", block_cases())
@pytest.mark.parametrize("batch", [1, 3, 256])
def test_token_half_batches_against_eager(name, batch):
    blk, _, _, _, sd, meta = hip_block(name)
    ref = build_block(meta, sd, eager_token_mixer).to(DEV)
    g = torch.Generator().manual_seed(batch)
    x = torch.randn(batch, meta["C"], meta["H"], meta["W"], generator=g)
    with torch.no_grad():
        want_r, want_t = token_half(ref, x.to(DEV))
        got_r, got_t = blk.token_half(cl(x))
        scale = max(1.0, float(want_t.abs().max()))
        assert float((got_r - want_r).abs().max()) <= 2e-4 * scale
        assert float((got_t - want_t).abs().max()) <= 2e-4 * scale
        xb = x.bfloat16()
        wr, wt = token_half(ref, xb.float().to(DEV))
        br, bt = blk.token_half(cl(xb))
        assert bf16_bar(br, wr.cpu()) and bf16_bar(bt, wt.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("name", block_cases())
def test_folded_and_unfolded_are_bit_identical(name):
    blk, x, _, _, _, _ = hip_block(name)
    fused = models.replace_batchnorm(copy.deepcopy(blk))
    assert isinstance(fused.rep_mixer, torch.nn.Conv2d)
    xs = cl(torch.cat([x, torch.randn(2, *x.shape[1:])]))
    with torch.no_grad():
        for dt in (torch.float32, torch.bfloat16):
            a = blk.token_half(xs.to(dt))
            b = fused.token_half(xs.to(dt))
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), dt


@pytest.mark.gpu
@pytest.mark.parametrize("name", block_cases())
def test_deterministic_and_batch_independent(name):
    blk, _, _, _, _, meta = hip_block(name)
    x = cl(torch.randn(6, meta["C"], meta["H"], meta["W"], generator=torch.Generator().manual_seed(7))).bfloat16()
    with torch.no_grad():
        r0, t0 = blk.token_half(x)
        for _ in range(40):
            r, t = blk.token_half(x)
            assert torch.equal(r, r0) and torch.equal(t, t0)
        parts = [blk.token_half(x[a:b]) for a, b in ((0, 1), (1, 4), (4, 6))]
    assert torch.equal(torch.cat([p[0] for p in parts]), r0) and torch.equal(torch.cat([p[1] for p in parts]), t0)


@pytest.mark.gpu
def test_argument_checks_raise_before_launch():
    blk, x, _, _, _, meta = hip_block("7x7_c256")
    s = meta["split"]
    with torch.no_grad():
        p = blk.packed_params()
        xg = cl(x)
        with pytest.raises(ValueError):
            ops.ls_recattn(xg.double(), *p, s)                         # dtype
        with pytest.raises(ValueError):
            ops.ls_recattn(xg[0], *p, s)                               # 3-D
        with pytest.raises(ValueError):
            ops.ls_recattn(xg, *p, s - 2)                              # split not in fours
        with pytest.raises(ValueError):
            ops.ls_recattn(cl(torch.randn(1, 252, 7, 7)), *p, s)       # packs sized for another C
        with pytest.raises(ValueError):
            ops.ls_recattn(xg, *p, s, heads=2)                         # no kernel
        bad = list(p)
        bad[4] = bad[4].to(torch.bfloat16)
        with pytest.raises(ValueError):
            ops.ls_recattn(xg, *bad, s)                                # a pack of the wrong dtype
        blk3, _, _, _, _, m3 = hip_block("4x4_c512")
        with pytest.raises(ValueError):
            ops.ls_la3(cl(torch.randn(1, 512, 9, 9)), *blk3.packed_params(), m3["split"], 1)     # 81 tokens


def _randomize_bn(net):
    for m in net.modules():
        if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.1)


def _pair(name):
    torch.manual_seed(0)
    ref = models.create_model(name, token_mixer=eager_token_mixer).eval()
    _randomize_bn(ref)
    net = models.create_model(name).eval()
    net.load_state_dict(ref.state_dict(), strict=True)
    return ref, net


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_launch_path_takes_only_the_new_entries(name, monkeypatch):
    _, net = _pair(name)
    net = net.to(DEV).to(memory_format=torch.channels_last)
    calls = {"ls": 0, "cat": 0, "other": 0}
    real = {k: getattr(ops, k) for k in ("ls_recattn", "ls_la3")}
    for k in real:
        monkeypatch.setattr(ops, k, lambda *a, _f=real[k], **kw: (calls.__setitem__("ls", calls["ls"] + 1), _f(*a, **kw))[1])
    for k in ("recattn2d", "recattn_down_qkcore", "recattn_qkcore", "linear_attention_core", "linear_attention_core_pe", "upadd_dwconv", "dwconv2d"):
        monkeypatch.setattr(ops, k, lambda *a, **kw: calls.__setitem__("other", calls["other"] + 1))
    real_cat = torch.cat
    monkeypatch.setattr(torch, "cat", lambda *a, **kw: (calls.__setitem__("cat", calls["cat"] + 1), real_cat(*a, **kw))[1])
    x = torch.randn(1, 3, 224, 224, device=DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        for dt in (torch.float32, torch.bfloat16):
            net.to(dt)(x.to(dt))
    blocks = sum(s[-1] for s in lsmodels.mixer_shapes(name))
    assert calls == {"ls": 2 * blocks, "cat": 0, "other": 0}, calls


def _check_models(ref, net, x):
    with torch.no_grad():
        a = ref(x)
        b = net(x.contiguous(memory_format=torch.channels_last))
        assert float((a - b).abs().max()) < 1e-3 * max(1.0, float(a.abs().max()))
        ab = copy.deepcopy(ref).bfloat16()(x.bfloat16()).float()
        bb = copy.deepcopy(net).bfloat16()(x.bfloat16().contiguous(memory_format=torch.channels_last)).float()
    scale = float(a.abs().max())
    assert float((bb - a).abs().max()) < 0.1 * scale + 0.05
    assert float((bb - a).abs().max()) <= 1.5 * float((ab - a).abs().max()) + 0.02 * scale
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_full_model_hip_vs_eager(name):
    ref, net = _pair(name)
    ref, net = ref.to(DEV), net.to(DEV).to(memory_format=torch.channels_last)
    x = torch.randn(2, 3, 224, 224, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    _check_models(ref, net, x)                                     # BatchNorms unfolded (the packs fold them)
    models.replace_batchnorm(ref)
    models.replace_batchnorm(net)
    _check_models(ref, net, x)
    # the serving path: GEMM-library pointwise convs and the fused channel mixer where it has a kernel (bf16)
    netb = copy.deepcopy(net).bfloat16()
    models.use_linear_pointwise(netb)
    models.pad_mlp_hidden(netb)
    assert models.use_fused_mlp(netb) > 0
    with torch.no_grad():
        a = ref(x)
        ab = copy.deepcopy(ref).bfloat16()(x.bfloat16()).float()
        bb = netb(x.bfloat16().contiguous(memory_format=torch.channels_last)).float()
    scale = float(a.abs().max())
    assert float((bb - a).abs().max()) < 0.1 * scale + 0.05
    assert float((bb - a).abs().max()) <= 1.5 * float((ab - a).abs().max()) + 0.02 * scale


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_full_model_at_256(name):
    ref, net = _pair(name)
    models.replace_batchnorm(ref)
    models.replace_batchnorm(net)
    ref, net = ref.to(DEV), net.to(DEV).to(memory_format=torch.channels_last)
    x = torch.randn(1, 3, 256, 256, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    with torch.no_grad():
        a, b = ref(x), net(x.contiguous(memory_format=torch.channels_last))
    assert float((a - b).abs().max()) < 1e-3 * max(1.0, float(a.abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_graph_replay_equals_eager(name):
    from recnext_amd.speed import build_inference_model
    net = build_inference_model(name, "cuda:0", torch.bfloat16)
    x = torch.randn(2, 3, 224, 224, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        want = net(x)
        run = GraphedInference(net)
        got = run(x)
        assert torch.equal(got, want)
        assert torch.equal(run(x), want)
