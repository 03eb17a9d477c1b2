"""GPU: RecAttn2d's coarse level on the matrix cores for heads of 36 .. 64 channels (RecNeXt-A5: 40 per head) -- rcx_recattn_qkcore_fwd in its one- and
two-launch forms, rcx_recattn_down_qkcore_fwd from 16-bit x, RecAttn2d at A5's stage sizes (no projection GEMM left in stages 0 - 2) and the whole
model against the ATen restatement."""
import copy

import numpy as np
import pytest
import torch

from recnext_amd import ops
from oracle import c_oracle
from tests.util import bf16_round_np
import tests.test_models as test_models
import tests.test_recconv_gpu as recconv_gpu

BF16_ATOL = BF16_RTOL = 1e-2
dev = recconv_gpu.dev


def _attn_params(rng, c):
    w_qk = (rng.standard_normal((2 * c, c // 2, 1, 1)) * (2.0 / c) ** 0.5).astype(np.float32)
    b_qk = (rng.standard_normal(2 * c) * 0.1).astype(np.float32)
    w_pe = (rng.standard_normal((c, 1, 3, 3)) * 0.2).astype(np.float32)
    b_pe = (rng.standard_normal(c) * 0.1).astype(np.float32)
    return w_qk, b_qk, w_pe, b_pe


def _worst(g, ref):
    return float((np.abs(g - ref) / (BF16_ATOL + BF16_RTOL * np.abs(ref))).max())


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(2, 80, 2, 28, 28), (4, 160, 4, 14, 14), (3, 320, 8, 7, 7),                      # A5's coarse planes, D = 40
                                  (2, 80, 2, 9, 11), (1, 80, 2, 1, 130), (1, 160, 4, 65, 1), (2, 80, 2, 5, 9), (2, 320, 8, 5, 9),
                                  (2, 96, 2, 28, 28), (2, 192, 4, 14, 14), (2, 384, 8, 7, 7),                          # D = 48
                                  (2, 128, 2, 28, 28), (2, 512, 8, 4, 4), (2, 512, 8, 7, 7),                           # D = 64 (7 x 7: two launches)
                                  (1, 72, 2, 56, 56), (2, 288, 8, 7, 7), (2, 240, 4, 7, 7)],                           # D = 36 / 36 / 60
                         ids=lambda c: "x".join(map(str, c)))
def test_recattn_qkcore_wide_heads(case):
    """rcx_recattn_qkcore_fwd with heads of 36 .. 64 channels against (a) the NumPy restatement of LinearAttention in float64 and (b) the float32
    two-step path (float32 GEMMs + the vector-pipe core), both within the 1e-2 bar of 16-bit runs; repeated launches are bit-identical and the call
    without the pe bias pack differs by exactly that bias."""
    from oracle import recconv_np
    b, c, heads, h, w = case
    assert ops.recattn_qkcore_supported(c, heads, h, w)
    rng = np.random.default_rng(c * 37 + h * w)
    d = rng.standard_normal((b, c, h, w)).astype(np.float32)
    w_qk, b_qk, w_pe, b_pe = _attn_params(rng, c)
    ref = recconv_np.linear_attention(d.astype(np.float64), w_qk, b_qk, w_pe, b_pe, heads, variant=1)
    t = lambda a: torch.from_numpy(a).to(dev())
    dd = t(d).contiguous(memory_format=torch.channels_last)
    wqk16 = t(w_qk[:, :, 0, 0]).to(torch.bfloat16).contiguous()
    wpe, bpe = ops.pack_dw_weight(t(w_pe)), ops.pack_bias(t(b_pe))
    got = ops.recattn_qkcore(dd, wqk16, t(b_qk), wpe, bpe, heads)
    assert got.dtype == torch.float32 and got.shape == dd.shape
    for _ in range(3):
        assert torch.equal(got, ops.recattn_qkcore(dd, wqk16, t(b_qk), wpe, bpe, heads)), "not deterministic"
    g = got.cpu().numpy()
    tok = dd.permute(0, 2, 3, 1).reshape(b * h * w, c)
    qpre = torch.nn.functional.linear(tok[:, :c // 2], t(w_qk[:c, :, 0, 0]), t(b_qk[:c])).view(b, h * w, c)
    kpre = torch.nn.functional.linear(tok[:, c // 2:], t(w_qk[c:, :, 0, 0]), t(b_qk[c:])).view(b, h * w, c)
    two = ops.linear_attention_core_pe(qpre, kpre, dd, wpe, bpe, heads)
    if two is None:
        two = ops.linear_attention_core(qpre, kpre, dd, ops.dwconv2d(dd, wpe, bpe, k=3, stride=1), heads)
    two = two.cpu().numpy()
    print(f"{'x'.join(map(str, case))}: launches {ops._lib.load().rcx_recattn_qkcore_launches(b, h, w, c, heads)}, max|err| vs float64 "
          f"{np.abs(g - ref).max():.3e} (float32 two-step {np.abs(two - ref).max():.3e}), worst err/tol {_worst(g, ref):.2f}")
    assert np.allclose(g, ref, atol=BF16_ATOL, rtol=BF16_RTOL)
    assert np.allclose(g, two, atol=BF16_ATOL, rtol=BF16_RTOL)
    nob = ops.recattn_qkcore(dd, wqk16, t(b_qk), wpe, None, heads).cpu().numpy()
    assert np.allclose(nob, g - b_pe[None, :, None, None], atol=1e-5, rtol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(3, 320, 8, 14), (2, 160, 4, 14), (2, 80, 2, 14), (2, 320, 8, 7), (2, 384, 8, 14), (2, 128, 2, 7)],
                         ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("xdt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_recattn_down_qkcore_wide_heads(case, xdt):
    """rcx_recattn_down_qkcore_fwd with heads of 36 .. 64 channels (A5 stage 2: 14 x 14, 8 heads of 40) against the C-oracle conv followed by the NumPy
    attention in float64, and against the two launches it replaces (rcx_dwconv2d_fwd + rcx_recattn_qkcore_fwd)."""
    from oracle import recconv_np
    b, c, heads, hw = case
    assert ops.recattn_down_qkcore_supported(c, heads, hw, hw, xdt)
    assert not ops.recattn_down_qkcore_supported(c, heads, hw, hw, torch.float32)
    assert not ops.recattn2d_supported(c, heads, hw, hw, "nearest", xdt)
    rng = np.random.default_rng(5 * c + hw)
    rnd = bf16_round_np if xdt == torch.bfloat16 else (lambda a: a.astype(np.float16).astype(np.float32))
    x = rnd(rng.standard_normal((b, c, hw, hw)).astype(np.float32))
    w_dn = (rng.standard_normal((c, 1, 5, 5)) * 0.2).astype(np.float32)
    b_dn = (rng.standard_normal(c) * 0.1).astype(np.float32)
    w_qk, b_qk, w_pe, b_pe = _attn_params(rng, c)
    ref = recconv_np.linear_attention(c_oracle.dwconv2d(x, w_dn, b_dn, 2).astype(np.float64), w_qk, b_qk, w_pe, b_pe, heads, variant=1)
    t = lambda a: torch.from_numpy(a).to(dev())
    xx = t(x).to(xdt).contiguous(memory_format=torch.channels_last)
    wdn, bdn, wpe, bpe = ops.pack_dw_weight(t(w_dn)), ops.pack_bias(t(b_dn)), ops.pack_dw_weight(t(w_pe)), ops.pack_bias(t(b_pe))
    wqk16 = t(w_qk[:, :, 0, 0]).to(torch.bfloat16).contiguous()
    got = ops.recattn_down_qkcore(xx, wdn, bdn, wqk16, t(b_qk), wpe, bpe, heads)
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape
    assert torch.equal(got, ops.recattn_down_qkcore(xx, wdn, bdn, wqk16, t(b_qk), wpe, bpe, heads)), "not deterministic"
    g = got.cpu().numpy()
    print(f"{'x'.join(map(str, case))}: worst err/tol vs the float64 oracle chain {_worst(g, ref):.2f}")
    assert np.allclose(g, ref, atol=BF16_ATOL, rtol=BF16_RTOL)
    two = ops.recattn_qkcore(ops.dwconv2d(xx, wdn, bdn, k=5, stride=2, out_dtype=torch.float32), wqk16, t(b_qk), wpe, bpe, heads)
    assert torch.allclose(got, two, atol=2e-3, rtol=2e-3), (got - two).abs().max().item()
    nob = ops.recattn_down_qkcore(xx, wdn, None, wqk16, t(b_qk), wpe, None, heads)
    two0 = ops.recattn_qkcore(ops.dwconv2d(xx, wdn, None, k=5, stride=2, out_dtype=torch.float32), wqk16, t(b_qk), wpe, None, heads)
    assert torch.allclose(nob, two0, atol=2e-3, rtol=2e-3)


def _spy(monkeypatch):
    """Count the calls of F.linear (the projection GEMMs) and of the matrix-core entry points during RecAttn2d.forward."""
    import recnext_amd.recattn as recattn_mod
    calls = {"linear": 0, "qkcore": 0, "down_qkcore": 0}

    def wrap(key, fn):
        def f(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return f
    monkeypatch.setattr(recattn_mod.F, "linear", wrap("linear", recattn_mod.F.linear))
    monkeypatch.setattr(ops, "recattn_qkcore", wrap("qkcore", ops.recattn_qkcore))
    monkeypatch.setattr(ops, "recattn_down_qkcore", wrap("down_qkcore", ops.recattn_down_qkcore))
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("stage,dim,hw,n", [(0, 80, 56, 32), (1, 160, 28, 256), (2, 320, 14, 256)], ids=["s0", "s1", "s2"])
def test_recattn2d_a5_stages_on_the_matrix_cores(stage, dim, hw, n, monkeypatch):
    """RecAttn2d at RecNeXt-A5's stage sizes (heads of 40), eval, bf16: no projection GEMM runs (the matrix-core kernels do), the output is deterministic
    and within the flat 1e-2 bar of the ATen restatement with non-trivial BatchNorm statistics; float32 x still takes the float32 GEMM chain."""
    from oracle.torch_eager import EagerRecAttn2d
    from recnext_amd.models import replace_batchnorm
    from recnext_amd.recattn import RecAttn2d
    heads = 2 ** (stage + 1)
    torch.manual_seed(stage)
    ref = EagerRecAttn2d(dim, num_heads=heads, stage=stage).eval()
    for m in ref.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5); m.weight.data.uniform_(0.6, 1.4); m.bias.data.normal_(0, 0.2)
    mod = RecAttn2d(dim, num_heads=heads, stage=stage).eval()
    mod.load_state_dict(ref.state_dict(), strict=True)
    x = torch.randn(n, dim, hw, hw, device=dev()).contiguous(memory_format=torch.channels_last)
    # float32 x: the GEMM chain, as before
    m32 = copy.deepcopy(mod).to(dev())
    calls = _spy(monkeypatch)
    with torch.no_grad():
        m32(x[:2])
    assert calls["linear"] == 2 and calls["qkcore"] == 0 and calls["down_qkcore"] == 0, calls
    # bf16 x: the matrix-core kernels, no GEMM
    mm = mod.to(dev()).to(torch.bfloat16)
    xb = x.to(torch.bfloat16)
    calls.update(linear=0, qkcore=0, down_qkcore=0)
    with torch.no_grad():
        y = mm(xb)
    assert calls["linear"] == 0 and calls["qkcore"] + calls["down_qkcore"] == 1, calls
    monkeypatch.undo()
    with torch.no_grad():
        assert torch.equal(mm(xb), y), "not deterministic"
    assert y.dtype == torch.bfloat16 and torch.isfinite(y.float()).all()
    idx = [0, n // 2, n - 1]
    ref_w = copy.deepcopy(ref).to(torch.bfloat16).float()
    with torch.no_grad():
        want = ref_w(xb[idx].float().cpu().contiguous())
        fused = copy.deepcopy(ref_w)
        replace_batchnorm(fused)
        assert float((want - fused(xb[idx].float().cpu().contiguous())).abs().max()) < 1e-4
        ref_bf16 = copy.deepcopy(ref).bfloat16()(xb[idx].cpu().contiguous()).float()
    recconv_gpu._assert_bf16_flat(y[idx].float().cpu().numpy(), want.numpy(), ref_bf16.numpy(), f"a5 stage {stage}")


@pytest.mark.gpu
def test_full_recnext_a5_hip_vs_eager():
    """The whole RecNeXt-A5 at 224, batch 2: HIP token mixers (the wide-head matrix-core kernels in its bf16 run) against the ATen restatement,
    float32 and bf16, with the bounds the other registered models meet."""
    test_models.test_full_model_hip_vs_eager_gpu("recnext_a5", 2)
