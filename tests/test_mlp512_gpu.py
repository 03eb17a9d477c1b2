"""The 512-channel channel mixer of the 7 x 7 stage in one launch (rcx_mlp.hip k_channel_mlp_wide: C = 512, H = 1024, offered from a token count M_min upward)
against the float64 formula on the same bf16 operands and against the four-launch library chain it replaces -- the assertions of
test_mlp_gpu.py::test_fused_channel_mlp_against_float64_and_the_gemm_path on shapes chosen from M_min, which is probed, not hard-coded."""
import pytest
import torch

from tests.mlp_common import check, dev, operands, reference

pytestmark = pytest.mark.gpu

C, HID = 512, 1024


def _m_min():
    """The smallest supported token count (the dispatch is a threshold: unsupported below, supported from it upward)."""
    from recnext_amd import ops
    lo, hi = 1024, 1 << 20                               # 1024 is pinned unsupported by test_mlp_gpu.py
    assert not ops.channel_mlp_supported(lo, C, HID, torch.bfloat16) and ops.channel_mlp_supported(hi, C, HID, torch.bfloat16)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ops.channel_mlp_supported(mid, C, HID, torch.bfloat16):
            hi = mid
        else:
            lo = mid
    return hi


def _cases():
    """(a) the smallest supported M in whole 7 x 7 images; (b) 5 x 9 images with M no multiple of 32: a ragged last workgroup (64 tokens) and a ragged token
    tile (32); (d) hidden 960, padded to 1024.  (The kernel does not loop over blocks: a workgroup per 64 tokens, so more workgroups than CUs is no other path.)"""
    m = _m_min()
    na = -(-m // 49)
    nb = -(-m // 45) + 1
    while nb % 32 == 0 or nb * 45 % 64 == 0:
        nb += 1
    return {"smallest": (na, C, HID, 7, 7), "ragged": (nb, C, HID, 5, 9), "hidden960": (na + 1, C, 960, 7, 7)}


@pytest.mark.parametrize("which", ["smallest", "ragged", "hidden960"])
def test_wide_channel_mlp_against_float64_and_the_gemm_path(which):
    from recnext_amd import ops
    case = _cases()[which]
    n, c, hid, h, w = case
    m = n * h * w
    assert ops.channel_mlp_supported(m, c, hid, torch.bfloat16)
    if which == "smallest":
        assert m - h * w < _m_min() <= m
    if which == "ragged":
        assert m % 64 and m % 32
    z, x, w1, b1, w2, b2 = operands(n, c, hid, h, w, seed=c * 1000 + hid + h)
    hp = ops.channel_mlp_hidden(m, c, hid, torch.bfloat16)
    assert hp == 1024
    wfrag, bias, hp2 = ops.pack_channel_mlp(w1, b1, w2, b2, hidden_to=hp)
    assert hp2 == hp
    y = ops.channel_mlp(z, x, wfrag, bias, hp)
    assert y.shape == x.shape and y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, ops.channel_mlp(z, x, wfrag, bias, hp)), "not deterministic"
    if which == "ragged":                                # exchange-buffer and barrier hazards would show as a launch that differs
        for _ in range(40):
            assert torch.equal(y, ops.channel_mlp(z, x, wfrag, bias, hp)), "not deterministic over repeated launches"
    ref = reference(z, x, w1, b1, w2, b2)
    err = check(y, ref, case)
    zz = z.permute(0, 2, 3, 1).reshape(-1, c)
    lib = torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(zz, w1, b1)), w2, b2)
    lib = x + lib.view(n, h, w, c).permute(0, 3, 1, 2)
    lib_err = (lib.double().cpu() - ref).abs()
    print(f"    mean |err| fused {float(err.mean()):.2e} / library {float(lib_err.mean()):.2e}; max {float(err.max()):.2e} / {float(lib_err.max()):.2e}")
    assert float(err.mean()) <= 1.05 * float(lib_err.mean()) + 1e-5 and float(err.max()) <= 1.25 * float(lib_err.max()) + 1e-3
    # Downsample's call: z and x are one tensor
    ref_alias = ops.channel_mlp(z, z.clone(), wfrag, bias, hp)
    assert torch.equal(ops.channel_mlp(z, z, wfrag, bias, hp), ref_alias)


def test_wide_channel_mlp_gelu_tails_are_exact():
    """test_mlp_gpu.py::test_fused_channel_mlp_gelu_tails_are_exact at (N, 512, 1024, 7, 7): exactly 0 below -6, only the bf16 roundings above +6."""
    from recnext_amd import ops
    n, c, hid, h, w = _cases()["smallest"]
    g = torch.Generator(device="cpu").manual_seed(7)
    z = (torch.randn(n, c, h, w, generator=g)).to(torch.bfloat16).to(dev()).contiguous(memory_format=torch.channels_last)
    x = torch.zeros_like(z)
    w1 = (torch.randn(hid, c, generator=g) * 40.0).to(torch.bfloat16).to(dev())
    b1 = torch.zeros(hid).to(torch.bfloat16).to(dev())
    w2 = torch.zeros(c, hid)
    w2[torch.arange(c), torch.arange(c)] = 1.0                                            # y[:, j] = gelu(hidden unit j)
    w2, b2 = w2.to(torch.bfloat16).to(dev()), torch.zeros(c).to(torch.bfloat16).to(dev())
    hp = ops.channel_mlp_hidden(n * h * w, c, hid, torch.bfloat16)
    assert hp == 1024
    wfrag, bias, _ = ops.pack_channel_mlp(w1, b1, w2, b2, hidden_to=hp)
    y = ops.channel_mlp(z, x, wfrag, bias, hp).float()
    pre = (z.float().permute(0, 2, 3, 1).reshape(-1, c) @ w1.float().t())[:, :c].reshape(n, h, w, c).permute(0, 3, 1, 2)
    assert float(pre.abs().max()) > 300.0
    neg = pre < -6.0
    assert bool(neg.any()) and float(y[neg].abs().max()) == 0.0, float(y[neg].abs().max())
    pos = pre > 6.0
    ref = pre.double().cpu()
    assert bool(((y.double().cpu() - ref)[pos.cpu()].abs() <= 8e-3 * ref[pos.cpu()].abs() + 1e-6).all())


def _count_fused(net, x):
    """(mixers whose forward took the fused launch, mixers in all) in one forward of net on x."""
    from recnext_amd import models
    hits, handles = [0, 0], []

    def hook(mod, inputs, output):
        fused = mod.__dict__.get("_fused_mlp")
        hits[1] += 1
        if fused is not None and not mod.training and fused.supported(output):
            hits[0] += 1

    for m in net.modules():
        if isinstance(m, (models.MetaNeXtBlock, models.Downsample)):
            handles.append(m.register_forward_hook(hook))
    with torch.no_grad():
        y = net(x)
    for hnd in handles:
        hnd.remove()
    return hits[0], hits[1], y.float()


def test_m3_runs_all_24_mixers_fused_above_m_min_and_the_library_below():
    from recnext_amd.speed import build_inference_model, synthetic_batch
    a = build_inference_model("recnext_m3", dev(), torch.bfloat16, seed=0, fused_mlp=False)
    b = build_inference_model("recnext_m3", dev(), torch.bfloat16, seed=0, fused_mlp=True)
    batch = -(-_m_min() // 49)
    x = synthetic_batch(batch, 224, dev(), torch.bfloat16, seed=1)
    fused, blocks, yb = _count_fused(b, x)
    assert (fused, blocks) == (24, 24)
    with torch.no_grad():
        ya = a(x).float()
    scale = float(ya.abs().max())
    assert float((ya - yb).abs().max()) < 0.05 * scale + 0.02, (float((ya - yb).abs().max()), scale)
    fused4, blocks4, _ = _count_fused(b, synthetic_batch(4, 224, dev(), torch.bfloat16, seed=1))
    assert (fused4, blocks4) == (21, 24)                 # batch 4: 196 tokens at 7 x 7 -- the GEMM library
