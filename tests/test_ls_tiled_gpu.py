"""GPU: the tiled token half of the LSNet-style RecNeXt-T / S / B (rcx_ls_recattn_tiled_fwd / rcx_ls_la3_tiled_fwd, rcx_lstile.hip): whole models
above 224 x 224 against the operator restatement, the large-plane reference fixtures, random blocks on tiny, ragged and large planes, the
one-workgroup entries where both exist, dispatch, determinism, shards, folding, graph replay and the argument checks.

Bars: those of tests/test_lsnet_gpu.py (imported, not restated) wherever the issue names them.  Two are derived here:
  * tiled against one-workgroup, float32: both evaluate the same float32 formula and differ in the order of the token sums and in where n^-1 is
    applied, a few roundings at the scale of the largest value: 8 float32 ulp of max(1, |t|max); r comes from the same taps in the same order: equal bits;
  * the same in 16-bit: two float32 values that differ by d round to outputs at most one output ulp + d apart.
"""
import copy

import pytest
import torch

from recnext_amd import lsmodels, models, ops
from recnext_amd.graph import GraphedInference
from tests.ls_eager import eager_token_mixer, token_half
from tests.test_ls_tiled_cpu import load_tiled_block, tiled_cases
from tests.test_lsnet_cpu import NAMES, block_cases, build_block, load_block
from tests.test_lsnet_gpu import DEV, _check_models, _pair, bf16_bar, cl

F32_ULPS = 8 * 2.0 ** -23
SIZES = [(288, 288), (384, 384), (512, 512), (320, 480)]
# random blocks: (fixture whose parameters the block takes, planes)
RANDOM_PLANES = {
    "12x12_c512": [(12, 12), (9, 13), (1, 1), (3, 5), (9, 9), (5, 13)],
    "36x36_c128": [(36, 36), (25, 19), (1, 1), (3, 5), (9, 9), (5, 13)],
    "16x16_c384": [(16, 16), (1, 1), (3, 5), (5, 13)],
    "25x19_c256": [(25, 19), (9, 9), (2, 65)],
}


def tiled_half(blk, x):
    """The tiled entry itself, whatever token_half would dispatch to."""
    attn = blk.token_mixer.attn
    s = blk.token_mixer.split_idx
    if isinstance(attn, lsmodels.LinearAttention3):
        return ops.ls_la3_tiled(x, *blk.packed_params(), s, attn.num_heads)
    return ops.ls_recattn_tiled(x, *blk.packed_params(), s, attn.down[1].num_heads)


def one_workgroup_half(blk, x):
    attn = blk.token_mixer.attn
    s = blk.token_mixer.split_idx
    if isinstance(attn, lsmodels.LinearAttention3):
        return ops.ls_la3(x, *blk.packed_params(), s, attn.num_heads)
    return ops.ls_recattn(x, *blk.packed_params(), s, attn.down[1].num_heads)


def tiled_block(name):
    x, r, t_s, sd, meta = load_tiled_block(name)
    return build_block(meta, sd).to(DEV), x, r, t_s, sd, meta


def ulp16(v, dt):
    """The spacing of `dt` (bf16: 8 significand bits, f16: 11) at |v|, float32 tensor in and out."""
    bits = 8 if dt == torch.bfloat16 else 11
    tiny = 2.0 ** -126 if dt == torch.bfloat16 else 2.0 ** -14
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(tiny))) - (bits - 1))


# ---- 1. whole models ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", NAMES)
def test_full_model_above_224(name, size):
    """recnext_s / _b at 512 x 512 raise NotImplementedError without the tiled entries (the 96-wide stage-2 slice at 16 x 16 has no other path); the
    smaller sizes ran on the library chain before and run on the tiled entries now."""
    ref, net = _pair(name)
    ref, net = ref.to(DEV), net.to(DEV).to(memory_format=torch.channels_last)
    x = torch.randn(1, 3, *size, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    _check_models(ref, net, x)
    models.replace_batchnorm(ref)
    models.replace_batchnorm(net)
    _check_models(ref, net, x)


@pytest.mark.gpu
def test_full_model_with_a_tiled_stage_3():
    """576 x 640: every stage of recnext_t, LinearAttention3's 9 x 10 plane included, is past the one-workgroup entries."""
    shapes = lsmodels.mixer_shapes("recnext_t", (576, 640))
    assert shapes[-1][1:3] == (9, 10) and not ops.ls_la3_supported(1, 9, 10, 512, 128, 1, torch.float32)
    ref, net = _pair("recnext_t")
    ref, net = ref.to(DEV), net.to(DEV).to(memory_format=torch.channels_last)
    x = torch.randn(1, 3, 576, 640, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    _check_models(ref, net, x)


# ---- 2. blocks ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", tiled_cases())
def test_token_half_matches_the_large_plane_fixture(name):
    blk, x, r, t_s, sd, meta = tiled_block(name)
    s, rc = meta["split"], meta["r_channels"]
    attn = blk.token_mixer.attn
    query = ops.ls_la3_supported if isinstance(attn, lsmodels.LinearAttention3) else ops.ls_recattn_supported
    heads = attn.num_heads if isinstance(attn, lsmodels.LinearAttention3) else 1
    assert not query(1, meta["H"], meta["W"], meta["C"], s, heads, torch.float32)        # token_half takes the tiled entry here
    with torch.no_grad():
        got_r, got_t = blk.token_half(cl(x))
        print(name, "fp32 |r| err", float((got_r[:, :rc].cpu() - r).abs().max()), "|t_s| err", float((got_t[:, :s].cpu() - t_s).abs().max()))
        assert float((got_r[:, :rc].cpu() - r).abs().max()) <= 2e-4
        assert float((got_t[:, :s].cpu() - t_s).abs().max()) <= 2e-4
        assert torch.equal(got_t[:, s:], got_r[:, s:])
        for dt in (torch.bfloat16, torch.float16):               # x is bf16-representable: the fixture is the float32 result on rounded input
            br, bt = blk.token_half(cl(x).to(dt))
            assert br.dtype == dt and bt.dtype == dt
            assert bf16_bar(br[:, :rc], r) and bf16_bar(bt[:, :s], t_s), dt
            assert torch.equal(bt[:, s:], br[:, s:])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RANDOM_PLANES))
@pytest.mark.parametrize("batch", [1, 3, 64])
def test_tiled_entry_against_eager(name, batch):
    blk, _, _, _, sd, meta = tiled_block(name)
    ref = build_block(meta, sd, eager_token_mixer).to(DEV)
    for (h, w) in RANDOM_PLANES[name]:
        g = torch.Generator().manual_seed(1000 * batch + 37 * h + w)
        x = torch.randn(batch, meta["C"], h, w, generator=g)
        with torch.no_grad():
            want_r, want_t = token_half(ref, x.to(DEV))
            got_r, got_t = tiled_half(blk, cl(x))
            scale = max(1.0, float(want_t.abs().max()))
            print(name, batch, (h, w), "fp32 err / bar", float((got_r - want_r).abs().max()) / (2e-4 * scale), float((got_t - want_t).abs().max()) / (2e-4 * scale))
            assert float((got_r - want_r).abs().max()) <= 2e-4 * scale, (h, w)
            assert float((got_t - want_t).abs().max()) <= 2e-4 * scale, (h, w)
            xb = x.bfloat16()
            wr, wt = token_half(ref, xb.float().to(DEV))
            br, bt = tiled_half(blk, cl(xb))
            assert bf16_bar(br, wr.cpu()) and bf16_bar(bt, wt.cpu()), (h, w)
            xh = x.half()
            wr, wt = token_half(ref, xh.float().to(DEV))
            hr, ht = tiled_half(blk, cl(xh))
            assert bf16_bar(hr, wr.cpu()) and bf16_bar(ht, wt.cpu()), (h, w)


# ---- 3. the same function where both entries exist ----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", block_cases())
def test_tiled_equals_one_workgroup(name):
    x, _, _, sd, meta = load_block(name)
    blk = build_block(meta, sd).to(DEV)
    xs = cl(torch.cat([x, torch.randn(2, *x.shape[1:], generator=torch.Generator().manual_seed(5))]))
    with torch.no_grad():
        r1, t1 = one_workgroup_half(blk, xs)
        r2, t2 = tiled_half(blk, xs)
        assert torch.equal(r1, r2)
        bound = F32_ULPS * max(1.0, float(t1.abs().max()))
        print(name, "fp32 tiled - one-workgroup", float((t1 - t2).abs().max()), "bound", bound)
        assert float((t1 - t2).abs().max()) <= bound
        for dt in (torch.bfloat16, torch.float16):
            r1, t1 = one_workgroup_half(blk, xs.to(dt))
            r2, t2 = tiled_half(blk, xs.to(dt))
            assert torch.equal(r1, r2), dt
            a, b = t1.float(), t2.float()
            assert bool(((a - b).abs() <= ulp16(torch.maximum(a.abs(), b.abs()), dt) + F32_ULPS * max(1.0, float(a.abs().max()))).all()), dt


# ---- 4. dispatch ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_launch_path_at_384_takes_only_the_hip_entries(name, monkeypatch):
    _, net = _pair(name)
    net = net.to(DEV).to(memory_format=torch.channels_last)
    calls = {"ls": 0, "tiled": 0, "cat": 0, "other": 0}

    def count(key, fn):
        return lambda *a, **kw: (calls.__setitem__(key, calls[key] + 1), fn(*a, **kw))[1]
    for k in ("ls_recattn", "ls_la3"):
        monkeypatch.setattr(ops, k, count("ls", getattr(ops, k)))
    for k in ("ls_recattn_tiled", "ls_la3_tiled"):
        monkeypatch.setattr(ops, k, count("tiled", getattr(ops, k)))
    for k in ("recattn2d", "recattn_down_qkcore", "recattn_qkcore", "linear_attention_core", "linear_attention_core_pe", "upadd_dwconv", "dwconv2d"):
        monkeypatch.setattr(ops, k, lambda *a, **kw: calls.__setitem__("other", calls["other"] + 1))
    monkeypatch.setattr(torch, "cat", count("cat", torch.cat))
    x = torch.randn(1, 3, 384, 384, device=DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        for dt in (torch.float32, torch.bfloat16):
            net.to(dt)(x.to(dt))
    ls = tiled = 0
    for (_, h, w, c, s, heads, kind, blocks) in lsmodels.mixer_shapes(name, 384):
        one = (ops.ls_la3_supported if kind == "la3" else ops.ls_recattn_supported)(1, h, w, c, s, heads, torch.bfloat16)
        ls, tiled = ls + (blocks if one else 0), tiled + (0 if one else blocks)
    assert calls == {"ls": 2 * ls, "tiled": 2 * tiled, "cat": 0, "other": 0}, calls
    assert tiled > 0 or name == "recnext_t"               # T's slices are narrow enough for one workgroup up to 24 x 24


# ---- 5. determinism, shards, folding ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name,plane", [("36x36_c128", (48, 48)), ("25x19_c256", (24, 24)), ("16x16_c384", (12, 12)), ("12x12_c512", (12, 12))])
def test_deterministic_at_full_size_and_batch_independent(name, plane):
    blk, _, _, _, _, meta = tiled_block(name)
    x = cl(torch.randn(64, meta["C"], *plane, generator=torch.Generator().manual_seed(7))).bfloat16()
    with torch.no_grad():
        r0, t0 = tiled_half(blk, x)
        for _ in range(50):
            r, t = tiled_half(blk, x)
            assert torch.equal(r, r0) and torch.equal(t, t0)
        parts = [tiled_half(blk, x[a:b].contiguous(memory_format=torch.channels_last)) for a, b in ((0, 1), (1, 4), (4, 37), (37, 64))]
        assert torch.equal(torch.cat([p[0] for p in parts]), r0) and torch.equal(torch.cat([p[1] for p in parts]), t0)
        xf = x[:5].float()
        rf, tf = tiled_half(blk, xf)
        one = [tiled_half(blk, xf[i:i + 1].contiguous(memory_format=torch.channels_last)) for i in range(5)]
        assert torch.equal(torch.cat([p[0] for p in one]), rf) and torch.equal(torch.cat([p[1] for p in one]), tf)


@pytest.mark.gpu
@pytest.mark.parametrize("name", tiled_cases())
def test_folded_and_unfolded_are_bit_identical(name):
    blk, x, _, _, _, _ = tiled_block(name)
    fused = models.replace_batchnorm(copy.deepcopy(blk))
    assert isinstance(fused.rep_mixer, torch.nn.Conv2d)
    xs = cl(torch.cat([x, torch.randn(2, *x.shape[1:])]))
    with torch.no_grad():
        for dt in (torch.float32, torch.bfloat16):
            a = blk.token_half(xs.to(dt))
            b = fused.token_half(xs.to(dt))
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), dt


# ---- 6. graph replay --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["recnext_t", "recnext_s"])
def test_graph_replay_at_384_equals_eager(name):
    """recnext_t as the issue asks; recnext_s because its stage 1 (24 x 24, 64-wide slice) is the one that takes a tiled entry at 384 x 384."""
    from recnext_amd.speed import build_inference_model
    net = build_inference_model(name, "cuda:0", torch.bfloat16)
    x = torch.randn(2, 3, 384, 384, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        want = net(x)
        run = GraphedInference(net)
        got = run(x)
        assert torch.equal(got, want)
        assert torch.equal(run(x), want)


# ---- 7. argument checks -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_argument_checks_raise_before_launch():
    blk, x, _, _, _, meta = tiled_block("36x36_c128")
    s = meta["split"]
    with torch.no_grad():
        p = blk.packed_params()
        xg = cl(x)
        with pytest.raises(ValueError):
            ops.ls_recattn_tiled(xg.double(), *p, s)                        # dtype
        with pytest.raises(ValueError):
            ops.ls_recattn_tiled(xg[0], *p, s)                              # 3-D
        with pytest.raises(ValueError):
            ops.ls_recattn_tiled(xg, *p, s - 2)                             # split not in fours
        with pytest.raises(ValueError):
            ops.ls_recattn_tiled(cl(torch.randn(1, 124, 36, 36)), *p, s)    # packs sized for another C
        with pytest.raises(ValueError):
            ops.ls_recattn_tiled(xg, *p, s, heads=2)                        # no kernel
        bad = list(p)
        bad[4] = bad[4].to(torch.bfloat16)
        with pytest.raises(ValueError):
            ops.ls_recattn_tiled(xg, *bad, s)                               # a pack of the wrong dtype
        short = torch.empty(36 * 36 * s, device=DEV)                        # the fine slice alone: no room for d, the result and the partials
        with pytest.raises(ValueError):
            ops.ls_recattn_tiled(xg, *p, s, workspace=short)
        with pytest.raises(ValueError):
            ops.ls_recattn_tiled(xg, *p, s, workspace=short.double())
        blk3, x3, _, _, _, m3 = tiled_block("12x12_c512")
        p3 = blk3.packed_params()
        with pytest.raises(ValueError):
            ops.ls_la3_tiled(cl(x3).double(), *p3, m3["split"], 1)
        with pytest.raises(ValueError):
            ops.ls_la3_tiled(cl(x3)[0], *p3, m3["split"], 1)
        with pytest.raises(ValueError):
            ops.ls_la3_tiled(cl(x3), *p3, m3["split"], 3)                   # split not a multiple of 2 heads
        with pytest.raises(ValueError):
            ops.ls_la3_tiled(cl(torch.randn(1, 256, 12, 12)), *p3, m3["split"], 1)
        with pytest.raises(ValueError):
            ops.ls_la3_tiled(cl(x3), *p3, m3["split"], 1, workspace=torch.empty(16, device=DEV))
        # a workspace of the caller's, larger than needed, is used as it is
        need = ops._lib.load().rcx_ls_la3_tiled_workspace_bytes(1, 12, 12, 512, m3["split"], 1, 0)
        a = ops.ls_la3_tiled(cl(x3), *p3, m3["split"], 1, workspace=torch.empty(need // 4 + 64, device=DEV))
        b = ops.ls_la3_tiled(cl(x3), *p3, m3["split"], 1)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
