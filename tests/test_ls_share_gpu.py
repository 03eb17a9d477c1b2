"""GPU: the share-channel RecNeXt-T / S / B (recnext_amd.lsshare).  The share block's one-launch token half (rcx_ls_share_fwd) against the
reference's fixtures and the operator restatement tests/ls_share_eager.py in three dtypes, with dense and channel-slice sources; bit-level checks
(r against ops.ls_la3_tiled's, repeat launches, batch shards, folding); guard bands; stage 2 on the tiled LinearAttention3 entry; the tiny model
and graph replay; whole models, their launch path and the fused channel mixer; training against float64 and a bf16-autocast step."""
import copy

import pytest
import torch
import torch.nn.functional as F

from recnext_amd import lsshare, models, ops
from recnext_amd.graph import GraphedInference
from tests import guard
from tests.ls_share_eager import eager_share_token_mixer, share_stage_forward, share_token_half
from tests.test_ls_share_cpu import NAMES, build_la3_block, build_share_block, load_la3_block, load_share_block, load_tiny, tiny
from tests.test_lsnet_gpu import _check_models, _randomize_bn, bf16_bar

DEV = torch.device("cuda:0")
# (B, H, W, C, split): one pixel (every tap but the centre out of bounds); every four-channel group from another source, odd and non-square; the
# models' own shape; the 7 x 7 plane; two sources of 12 channels
SHAPES = [(1, 1, 1, 16, 4), (2, 3, 5, 16, 4), (3, 4, 4, 512, 128), (2, 7, 7, 512, 128), (1, 14, 9, 24, 12)]
IDS = ["x".join(str(v) for v in s) for s in SHAPES]


def cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _block(c, seed):
    """A share block with non-trivial BatchNorm statistics, and the same block on library operators."""
    torch.manual_seed(seed)
    ref = lsshare.ShareBlock(c, 1.5, hip=False).eval()
    _randomize_bn(ref)
    hip = lsshare.ShareBlock(c, 1.5).eval()
    hip.load_state_dict(ref.state_dict(), strict=True)
    return ref.to(DEV).requires_grad_(False), hip.to(DEV).requires_grad_(False)


def _inputs(shape, seed):
    """x and C / split sources of different data (bf16-representable), on the CPU in float32."""
    b, h, w, c, s = shape
    g = torch.Generator().manual_seed(seed)
    mk = lambda ch: torch.randn(b, ch, h, w, generator=g).bfloat16().float()
    return mk(c), [mk(s) for _ in range(c // s)]


def _as_views(srcs, c, dtype):
    """Each source as t_prev[:, :split] of a C-channel channels_last tensor whose other channels hold NaN."""
    out = []
    for s in srcs:
        full = torch.full((s.shape[0], c, s.shape[2], s.shape[3]), float("nan"), dtype=dtype, device=DEV).contiguous(memory_format=torch.channels_last)
        full[:, :s.shape[1]] = s.to(DEV).to(dtype)
        out.append(full[:, :s.shape[1]])
    return out


def _as_dense(srcs, dtype):
    return [cl(s).to(dtype) for s in srcs]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kernel_against_the_eager_form(shape):
    b, h, w, c, s = shape
    ref, hip = _block(c, seed=c + h)
    x, srcs = _inputs(shape, seed=h * w)
    wr, br = hip.packed_params()
    with torch.no_grad():
        want_r, want_t = share_token_half(ref, x.to(DEV), [v.to(DEV) for v in srcs])        # float32 on bf16-representable inputs
        scale = max(1.0, float(want_t.abs().max()))
        for form in ("dense", "views"):
            mk = (lambda dt: _as_dense(srcs, dt)) if form == "dense" else (lambda dt: _as_views(srcs, c, dt))
            r, t = lsshare.ls_share(cl(x), wr, br, mk(torch.float32))
            er, et = float((r - want_r).abs().max()), float((t - want_t).abs().max())
            print(f"ls_share {shape} {form} float32: |r err| {er:.3e} |t err| {et:.3e} (bar {2e-4 * scale:.3e})")
            assert r.shape == x.shape and r.is_contiguous(memory_format=torch.channels_last) and t.is_contiguous(memory_format=torch.channels_last)
            assert not bool(torch.isnan(t).any()) and not bool(torch.isnan(r).any()), form
            assert er <= 2e-4 * scale and et <= 2e-4 * scale, form
            for dt in (torch.bfloat16, torch.float16):
                br_, bt_ = lsshare.ls_share(cl(x).to(dt), wr, br, mk(dt))
                assert br_.dtype == dt and bt_.dtype == dt
                assert not bool(torch.isnan(bt_).any()), (form, dt)
                assert bf16_bar(br_, want_r.cpu()) and bf16_bar(bt_, want_t.cpu()), (form, dt)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["4x4_c512", "3x5_c16"])
def test_share_block_matches_the_fixture(name):
    x, x1s, r, t, sd, meta = load_share_block(name)
    blk = build_share_block(meta, sd).to(DEV).requires_grad_(False)
    c = meta["C"]
    with torch.no_grad():
        for mk in (_as_dense, lambda s, dt: _as_views(s, c, dt)):
            got_r, got_t = blk.token_half(cl(x), mk(x1s, torch.float32))
            assert float((got_r.cpu() - r).abs().max()) <= 2e-4 * max(1.0, float(r.abs().max()))
            assert float((got_t.cpu() - t).abs().max()) <= 2e-4 * max(1.0, float(t.abs().max()))
            for dt in (torch.bfloat16, torch.float16):          # x and the sources are bf16-representable: the fixture is the float32 result on rounded input
                br, bt = blk.token_half(cl(x).to(dt), mk(x1s, dt))
                assert br.dtype == dt and bf16_bar(br, r) and bf16_bar(bt, t), dt


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 4, 4, 512, 128), (1, 3, 5, 16, 4)], ids=["2x4x4x512", "1x3x5x16"])
def test_r_has_the_bits_of_the_tiled_token_half(shape):
    b, h, w, c, s = shape
    _, hip = _block(c, seed=3)
    torch.manual_seed(4)
    mixer = lsshare.MetaNeXtBlock(c, 1.5, stage=3).eval()
    _randomize_bn(mixer)
    mixer.rep_mixer.load_state_dict(hip.rep_mixer.state_dict())
    mixer = mixer.to(DEV).requires_grad_(False)
    x, srcs = _inputs(shape, seed=9)
    with torch.no_grad():
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            r, _ = lsshare.ls_share(cl(x).to(dt), *hip.packed_params(), _as_views(srcs, c, dt))
            pack = [p.clone() for p in mixer.packed_params()]       # fresh allocations: at split 4 the module's two-element k bias is a view 8 bytes into its tensor
            r_tiled, _ = ops.ls_la3_tiled(cl(x).to(dt), *pack, s, 1)
            assert torch.equal(r, r_tiled), dt


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(6, 4, 4, 512, 128), (6, 3, 5, 16, 4)], ids=["6x4x4x512", "6x3x5x16"])
def test_deterministic_and_batch_independent(shape):
    b, h, w, c, s = shape
    _, hip = _block(c, seed=5)
    x, srcs = _inputs(shape, seed=11)
    pack = hip.packed_params()
    with torch.no_grad():
        for dt in (torch.float32, torch.bfloat16):
            xs, vs = cl(x).to(dt), _as_views(srcs, c, dt)
            r0, t0 = lsshare.ls_share(xs, *pack, vs)
            r1, t1 = lsshare.ls_share(xs, *pack, vs)
            assert torch.equal(r0, r1) and torch.equal(t0, t1)
            parts = [lsshare.ls_share(xs[i:i + 1], *pack, [v[i:i + 1] for v in vs]) for i in range(b)]
            assert torch.equal(torch.cat([p[0] for p in parts]), r0) and torch.equal(torch.cat([p[1] for p in parts]), t0)


@pytest.mark.gpu
def test_folded_and_unfolded_are_bit_identical():
    _, hip = _block(512, seed=6)
    fused = models.replace_batchnorm(copy.deepcopy(hip))
    assert isinstance(fused.rep_mixer, torch.nn.Conv2d)
    shape = (3, 4, 4, 512, 128)
    x, srcs = _inputs(shape, seed=12)
    with torch.no_grad():
        for dt in (torch.float32, torch.bfloat16):
            vs = _as_views(srcs, 512, dt)
            a = hip.token_half(cl(x).to(dt), vs)
            b = fused.token_half(cl(x).to(dt), vs)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), dt


@pytest.mark.gpu
def test_unsupported_shapes_and_gpu_argument_checks_raise():
    _, hip = _block(16, seed=7)
    x, srcs = _inputs((2, 3, 5, 16, 4), seed=13)
    wr, br = hip.packed_params()
    with torch.no_grad():
        with pytest.raises(ValueError, match="source 1"):
            lsshare.ls_share(cl(x), wr, br, [cl(srcs[0]), srcs[1]] + _as_dense(srcs[2:], torch.float32))       # a source on the CPU
        with pytest.raises(ValueError, match="w_rep"):
            lsshare.ls_share(cl(x), wr.cpu(), br, _as_dense(srcs, torch.float32))
        nine = [cl(torch.zeros(1, 4, 2, 2)) for _ in range(9)]
        with pytest.raises(ValueError, match="1 .. 8"):
            lsshare.ls_share(cl(torch.zeros(1, 36, 2, 2)), torch.zeros(9 * 36, device=DEV), torch.zeros(36, device=DEV), nine)
        _, hip36 = _block(36, seed=8)
        with pytest.raises(ValueError, match="x1s is empty"):
            hip36.token_half(cl(torch.zeros(1, 36, 2, 2)), [])
        six = [cl(torch.zeros(1, 6, 2, 2)) for _ in range(6)]                                                   # split 6: no kernel, no fallback
        with pytest.raises(NotImplementedError, match="no kernel"):
            hip36.token_half(cl(torch.zeros(1, 36, 2, 2)), six)


def _guard_args(shape, dtype, seed):
    b, h, w, c, s = shape
    _, hip = _block(c, seed=seed)
    x, srcs = _inputs(shape, seed=seed + 1)
    return hip, (cl(x).to(dtype), *hip.packed_params(), _as_views(srcs, c, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 16, 4), (2, 4, 4, 512, 128)], ids=["2x3x5x16", "2x4x4x512"])
def test_guard_bands(shape, dtype):
    """Properties A - D of tests/guard.py for the entry and for a share block's token_half through the module: nothing outside r and t is written,
    every element of both is, nothing outside x, the pack and the first `split` channels of each source pixel is read (the guarded copy of a view
    source keeps its strides: the gaps hold the guard byte, 0x00 then 0xFF), and no input changes."""
    with torch.no_grad():
        hip, args = _guard_args(shape, dtype, seed=20)
        guard.run_properties(lambda x, wr, br, srcs: lsshare.ls_share(x, wr, br, srcs), args, modules=[lsshare, "recnext_amd.ops"])
        # through the module: the pack is the module's own (an allocation of the library, not an input)
        guard.run_properties(lambda x, srcs: hip.token_half(x, srcs), (args[0], args[3]), modules=[lsshare, "recnext_amd.ops", "recnext_amd.lsmodels"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["14x14_c256", "14x14_c384"])
def test_stage2_token_half_goes_to_the_tiled_entry_and_matches_the_fixture(name, monkeypatch):
    x, r, t_s, sd, meta = load_la3_block(name)
    blk = build_la3_block(meta, sd).to(DEV).requires_grad_(False)
    calls = {"tiled": 0, "one": 0}
    real = ops.ls_la3_tiled
    monkeypatch.setattr(ops, "ls_la3_tiled", lambda *a, **kw: (calls.__setitem__("tiled", calls["tiled"] + 1), real(*a, **kw))[1])
    monkeypatch.setattr(ops, "ls_la3", lambda *a, **kw: calls.__setitem__("one", calls["one"] + 1))
    s = meta["split"]
    with torch.no_grad():
        got_r, got_t = blk.token_half(cl(x))
        assert float((got_r.cpu() - r).abs().max()) <= 2e-4
        assert float((got_t[:, :s].cpu() - t_s).abs().max()) <= 2e-4
        assert torch.equal(got_t[:, s:], got_r[:, s:])
        for dt in (torch.bfloat16, torch.float16):
            br, bt = blk.token_half(cl(x).to(dt))
            assert br.dtype == dt and bt.dtype == dt
            assert bf16_bar(br, r) and bf16_bar(bt[:, :s], t_s), dt
            assert torch.equal(bt[:, s:], br[:, s:])
    assert calls == {"tiled": 3, "one": 0}


@pytest.mark.gpu
def test_tiny_model_reproduces_the_fixture_logits_and_graph_replay():
    x, logits, logits_fused, sd = load_tiny()
    net = tiny()
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).to(memory_format=torch.channels_last).requires_grad_(False)
    xs = cl(x)
    bar = lambda a: 1e-3 * max(1.0, float(a.abs().max()))
    with torch.no_grad():
        got = net(xs)
        assert float((got.cpu() - logits).abs().max()) < bar(logits)
        models.replace_batchnorm(net)
        got = net(xs)
        assert float((got.cpu() - logits_fused).abs().max()) < bar(logits_fused)
        # graph replay against the plain forward, bit for bit.  The 1x1 convs go to the GEMM library first, as in every served model: the conv
        # library's float32 1x1 convs differ from run to run in the last bit (two plain forwards do), with or without a graph.
        models.use_linear_pointwise(net)
        for m, xx in ((net, xs), (copy.deepcopy(net).bfloat16(), xs.bfloat16())):
            want = m(xx)
            run = GraphedInference(m)
            assert torch.equal(run(xx), want)
            assert torch.equal(run(xx), want)
        assert float((net(xs).cpu() - logits_fused).abs().max()) < bar(logits_fused)


def _pair(name):
    torch.manual_seed(0)
    ref = models.create_model(name, token_mixer=eager_share_token_mixer).eval()
    _randomize_bn(ref)
    net = models.create_model(name).eval()
    net.load_state_dict(ref.state_dict(), strict=True)
    return ref.requires_grad_(False), net.requires_grad_(False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_full_model_hip_vs_eager_and_its_launch_path(name, monkeypatch):
    ref, net = _pair(name)
    ref, net = ref.to(DEV), net.to(DEV).to(memory_format=torch.channels_last)
    x = torch.randn(2, 3, 224, 224, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    _check_models(ref, net, x)                                     # BatchNorms unfolded (the packs fold them); float32 and bf16
    models.replace_batchnorm(ref)
    models.replace_batchnorm(net)
    _check_models(ref, net, x)
    # per forward: two share launches, the slice mixers on the token-half entries, no concatenation and no library operator in a token half
    calls = {"share": 0, "ls": 0, "cat": 0, "other": 0}
    real_share = lsshare.ls_share
    monkeypatch.setattr(lsshare, "ls_share", lambda *a, **kw: (calls.__setitem__("share", calls["share"] + 1), real_share(*a, **kw))[1])
    for k in ("ls_recattn", "ls_la3", "ls_recattn_tiled", "ls_la3_tiled"):
        monkeypatch.setattr(ops, k, lambda *a, _f=getattr(ops, k), **kw: (calls.__setitem__("ls", calls["ls"] + 1), _f(*a, **kw))[1])
    for k in ("recattn2d", "recattn_down_qkcore", "recattn_qkcore", "linear_attention_core", "linear_attention_core_pe", "upadd_dwconv", "dwconv2d"):
        monkeypatch.setattr(ops, k, lambda *a, **kw: calls.__setitem__("other", calls["other"] + 1))
    real_cat = torch.cat
    monkeypatch.setattr(lsshare.torch, "cat", lambda *a, **kw: (calls.__setitem__("cat", calls["cat"] + 1), real_cat(*a, **kw))[1])
    xs = x.contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        net(xs)
        assert calls == {"share": 2, "ls": sum(s[-1] for s in lsshare.mixer_shapes(name) if s[6] != "share"), "cat": 0, "other": 0}, calls
        net.bfloat16()(xs.bfloat16())
        assert calls["share"] == 4 and calls["cat"] == 0 and calls["other"] == 0, calls


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_serving_path_fuses_every_stage3_channel_mixer(name, monkeypatch):
    from recnext_amd.speed import build_inference_model
    net = build_inference_model(name, "cuda:0", torch.bfloat16, fused_mlp=True)
    blocks = list(net.stages[3].blocks)
    assert all(b.__dict__.get("_fused_mlp") is not None for b in blocks) and sum(b.is_share_block for b in blocks) == 2
    seen = []
    real = ops.channel_mlp
    monkeypatch.setattr(ops, "channel_mlp", lambda z, x, *a, **kw: (seen.append((tuple(z.shape), z.data_ptr())), real(z, x, *a, **kw))[1])
    halves = []
    for b in blocks:                                               # every stage-3 block's t, as its token half hands it to the channel mixer
        orig = b.token_half
        b.token_half = lambda *a, _f=orig, **kw: (lambda rt: (halves.append(rt[1].data_ptr()), rt)[1])(_f(*a, **kw))
    x = torch.randn(32, 3, 224, 224, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        y = net(x)
        assert sum(shape == (32, 512, 4, 4) for shape, _ in seen) == len(blocks) + 1          # the blocks and the stage's Downsample
        run = GraphedInference(net)                                # the serving path replays as a graph, the list of views included
        for b in blocks:
            del b.token_half
        want = net(x)
        assert torch.equal(run(x), want) and torch.equal(y, want)
    fused = {p for shape, p in seen if shape == (32, 512, 4, 4)}
    assert len(halves) == len(blocks) and set(halves) <= fused     # each of them, share blocks included, went through the fused launch
    assert bool(torch.isfinite(y.float()).all())


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _stage_pair(seed):
    """A tiny share stage (C = 64, split 16, depth 6: four mixer blocks, the share block, a trailing mixer block) on HIP in float32 and its
    restatement in float64, the same parameters, train mode."""
    torch.manual_seed(seed)
    kw = dict(depth=6, mlp_ratio=1.5, downsample=False, stage=3, split_rate=4)
    ref = lsshare.RecNextStage(64, 64, token_mixer=eager_share_token_mixer, **kw)
    g = torch.Generator().manual_seed(seed)
    for m in ref.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.3)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 0.8 + 0.4)
            m.weight.data.copy_(torch.rand(m.weight.shape, generator=g) * 0.8 + 0.6)
            m.bias.data.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
    hip = lsshare.RecNextStage(64, 64, **kw)
    hip.load_state_dict(ref.state_dict(), strict=True)
    assert [b.is_share_block for b in hip.blocks] == [False] * 4 + [True, False]
    return ref.double().to(DEV).train(), hip.to(DEV).train()


@pytest.mark.gpu
def test_share_stage_training_matches_the_float64_restatement():
    """Train mode, batch statistics: HIP in float32 against the restatement in float64, with the bars tests/test_ls_train_gpu.py has for its float64
    comparisons (test_block_training_matches_reference_fixture): relative 1e-4 for r / t, 2e-3 for gx and the parameter gradients, or within 3x the
    float32 operator chain's own distance from float64.  The second clause decides here: RepVGGDW's depthwise 1x1 `sk` is x * w + b in front of a
    train-mode BatchNorm, and a channel whose |w| is small (0.0016 at this seed) loses its digits when the batch mean is taken off, in any float32
    implementation.  Measured on an MI355X, the same to three digits for HIP and for the float32 chain: r / t of the six blocks 1.3e-4 .. 4.7e-4,
    gx 4.3e-4, sk.conv.weight gradients of blocks 0-2 at 5.8 / 2.4 / 1.1 times the 2e-3 bar."""
    ref, hip = _stage_pair(seed=31)
    ref32 = copy.deepcopy(ref).float()
    g = torch.Generator(device=DEV).manual_seed(32)
    x = torch.randn(3, 64, 4, 4, device=DEV, generator=g).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(3, 64, 4, 4, device=DEV, generator=g)

    def restated(net, xx, gg):
        xx = xx.clone().requires_grad_(True)
        halves = []
        y = share_stage_forward(net, xx, halves)
        (y * gg).sum().backward()
        return y, xx.grad, halves

    y64, gx64, halves64 = restated(ref, x.double(), gy.double())
    y32, gx32, halves32 = restated(ref32, x, gy)
    # HIP, float32: every block's (r, t) as its token half returns them
    halves = []
    for b in hip.blocks:
        orig = b.token_half
        b.token_half = lambda *a, _f=orig, **kw: (lambda rt: (halves.append(rt), rt)[1])(_f(*a, **kw))
    xh = x.clone().requires_grad_(True)
    y = hip(xh)
    (y * gy).sum().backward()

    dist = lambda got, want: float((got.detach().double() - want.detach()).abs().max())

    def within(got, chain, want, rel, what):
        top = float(want.detach().abs().max())
        bar = max(rel * top, 3 * dist(chain, want))
        print(f"{what}: HIP {dist(got, want):.3e} float32 chain {dist(chain, want):.3e} bar {bar:.3e} ({rel:g} relative: {rel * top:.3e})")
        assert dist(got, want) <= bar, what

    assert len(halves) == len(halves64) == 6
    for i, ((r, t), (r32, t32), (r64, t64)) in enumerate(zip(halves, halves32, halves64)):
        within(r, r32, r64, 1e-4, f"block {i} r")
        within(t, t32, t64, 1e-4, f"block {i} t")
        assert t.is_contiguous(memory_format=torch.channels_last)
    within(y, y32, y64, 1e-4, "stage output")
    within(xh.grad, gx32, gx64, 2e-3, "gx")
    pr, p32, ph = dict(ref.named_parameters()), dict(ref32.named_parameters()), dict(hip.named_parameters())
    scale = max(float(p.grad.abs().max()) for p in pr.values() if p.grad is not None)
    for k, p in pr.items():
        if p.grad is None:                                         # read by nobody: the same on both sides
            assert ph[k].grad is None or not bool(ph[k].grad.any()), k
            continue
        assert ph[k].grad is not None, k
        assert dist(ph[k].grad, p.grad) <= max(2e-3 * float(p.grad.abs().max()) + 1e-5 * scale, 3 * dist(p32[k].grad, p.grad)), k
    for i in range(4):                                             # the gradient reaches the four mixer blocks' slice mixers (through their own t and the share block's)
        for k, p in hip.blocks[i].token_mixer.attn.named_parameters():
            assert p.grad is not None and bool(p.grad.any()), (i, k)
    for k, p in ref.blocks[5].token_mixer.attn.named_parameters():  # the trailing block: whatever the restatement's autograd says
        q = dict(hip.blocks[5].token_mixer.attn.named_parameters())[k]
        assert (p.grad is None or not bool(p.grad.any())) == (q.grad is None or not bool(q.grad.any())), k
    for (k, b64), (_, bh) in zip(ref.named_buffers(), hip.named_buffers()):
        assert torch.allclose(b64.float(), bh.float(), atol=1e-5, rtol=1e-4), k


@pytest.mark.gpu
def test_the_share_block_carries_the_gradient_to_the_slice_mixers():
    """A loss on the share block's t alone: its only way to the four mixer blocks' slice mixers is through the sources."""
    _, hip = _stage_pair(seed=33)
    x = torch.randn(3, 64, 4, 4, device=DEV).contiguous(memory_format=torch.channels_last)
    kept = []
    orig = hip.blocks[4].token_half
    hip.blocks[4].token_half = lambda *a, **kw: (lambda rt: (kept.append(rt), rt)[1])(orig(*a, **kw))
    hip(x)
    r, t = kept[0]
    (t - r).square().sum().backward()                              # t - r = cat(x1s): block 3's x1 reaches it only through the list
    for k, p in hip.blocks[3].token_mixer.attn.named_parameters():
        if k.endswith("norm.weight") or k.endswith("norm.bias") or k == "pe.conv.weight":      # (a conv bias in front of a train-mode BatchNorm has none)
            assert p.grad is not None and bool(p.grad.any()), k
    assert all(p.grad is None for p in hip.blocks[5].parameters())


@pytest.mark.gpu
def test_bf16_autocast_step_of_the_tiny_model():
    _, _, _, sd = load_tiny()
    ref, hip = tiny(eager_share_token_mixer), tiny()
    ref.load_state_dict(sd, strict=True)
    hip.load_state_dict(sd, strict=True)
    ref, hip = ref.to(DEV).train(), hip.to(DEV).to(memory_format=torch.channels_last).train()
    g = torch.Generator(device=DEV).manual_seed(6)
    x = torch.randn(4, 3, 128, 128, device=DEV, generator=g)
    y = torch.randint(0, 10, (4,), device=DEV, generator=g)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lr = F.cross_entropy(ref(x), y)
        lh = F.cross_entropy(hip(x.contiguous(memory_format=torch.channels_last)), y)
    lr.backward(), lh.backward()
    print(f"bf16 autocast loss: eager {float(lr.detach()):.5f} HIP {float(lh.detach()):.5f}")
    assert bool(torch.isfinite(lh)) and abs(float(lh.detach()) - float(lr.detach())) < 5e-2 * max(1.0, abs(float(lr.detach())))
    for k, p in hip.named_parameters():
        assert p.grad is None or bool(torch.isfinite(p.grad).all()), k
