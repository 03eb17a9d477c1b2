"""The channel mixers of RecNeXt-T / S / B (and of M1 / A1's 7 x 7 stage) in one launch: (C, hidden) = (512, 768) and (384, 768) on rcx_mlp.hip
k_channel_mlp_wide, each offered from a token count M_min upward -- the assertions of test_mlp512_gpu.py at each shape, on cases chosen from M_min, which is
probed, not hard-coded."""
import functools

import pytest
import torch

from tests.mlp_common import check, dev, operands, reference

pytestmark = pytest.mark.gpu

HID = 768
PLANE = {512: (4, 4), 384: (7, 7)}                      # the plane the shape has in the models at 224 x 224
SHAPES = sorted(PLANE)


@functools.lru_cache(maxsize=None)
def _m_min(c):
    """The smallest supported token count (the dispatch is a threshold: unsupported below, supported from it upward)."""
    from recnext_amd import ops
    lo, hi = 0, 1 << 20
    assert not ops.channel_mlp_supported(lo, c, HID, torch.bfloat16) and ops.channel_mlp_supported(hi, c, HID, torch.bfloat16)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ops.channel_mlp_supported(mid, c, HID, torch.bfloat16):
            hi = mid
        else:
            lo = mid
    return hi


def _cases(c):
    """(a) the smallest supported M in whole planes of the models; (b) 5 x 9 planes with M no multiple of 32: a ragged last workgroup (64 tokens) and a ragged
    token tile (32); (c) hidden 750, padded to 768.  (The kernel does not loop over blocks: a workgroup per 64 tokens, so more workgroups than CUs is no other path.)"""
    m = _m_min(c)
    ph, pw = PLANE[c]
    na = -(-m // (ph * pw))
    nb = -(-m // 45) + 1
    while nb % 32 == 0 or nb * 45 % 64 == 0 or nb * 45 % 32 == 0:
        nb += 1
    return {"smallest": (na, c, HID, ph, pw), "ragged": (nb, c, HID, 5, 9), "hidden750": (na + 1, c, 750, ph, pw)}


@pytest.mark.parametrize("which", ["smallest", "ragged", "hidden750"])
@pytest.mark.parametrize("c", SHAPES)
def test_wide_channel_mlp_against_float64_and_the_gemm_path(c, which):
    from recnext_amd import ops
    case = _cases(c)[which]
    n, _, hid, h, w = case
    m = n * h * w
    assert ops.channel_mlp_supported(m, c, hid, torch.bfloat16)
    if which == "smallest":
        assert m - h * w < _m_min(c) <= m
    if which == "ragged":
        assert m % 64 and m % 32
    z, x, w1, b1, w2, b2 = operands(n, c, hid, h, w, seed=c * 1000 + hid + h)
    hp = ops.channel_mlp_hidden(m, c, hid, torch.bfloat16)
    assert hp == 768
    wfrag, bias, hp2 = ops.pack_channel_mlp(w1, b1, w2, b2, hidden_to=hp)
    assert hp2 == hp
    y = ops.channel_mlp(z, x, wfrag, bias, hp)
    assert y.shape == x.shape and y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, ops.channel_mlp(z, x, wfrag, bias, hp)), "not deterministic"
    if which == "ragged":                                # an exchange-buffer or barrier hazard (three steps, six owning waves) would show as a launch that differs
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


@pytest.mark.parametrize("c", SHAPES)
def test_wide_channel_mlp_gelu_tails_are_exact(c):
    """test_mlp_gpu.py::test_fused_channel_mlp_gelu_tails_are_exact at (N, C, 768, plane): exactly 0 below -6, only the bf16 roundings above +6."""
    from recnext_amd import ops
    n, _, hid, h, w = _cases(c)["smallest"]
    g = torch.Generator(device="cpu").manual_seed(7)
    z = (torch.randn(n, c, h, w, generator=g)).to(torch.bfloat16).to(dev()).contiguous(memory_format=torch.channels_last)
    x = torch.zeros_like(z)
    w1 = (torch.randn(hid, c, generator=g) * 40.0).to(torch.bfloat16).to(dev())
    b1 = torch.zeros(hid).to(torch.bfloat16).to(dev())
    w2 = torch.zeros(c, hid)
    w2[torch.arange(c), torch.arange(c)] = 1.0                                            # y[:, j] = gelu(hidden unit j)
    w2, b2 = w2.to(torch.bfloat16).to(dev()), torch.zeros(c).to(torch.bfloat16).to(dev())
    hp = ops.channel_mlp_hidden(n * h * w, c, hid, torch.bfloat16)
    assert hp == 768
    wfrag, bias, _ = ops.pack_channel_mlp(w1, b1, w2, b2, hidden_to=hp)
    y = ops.channel_mlp(z, x, wfrag, bias, hp).float()
    pre = (z.float().permute(0, 2, 3, 1).reshape(-1, c) @ w1.float().t())[:, :c].reshape(n, h, w, c).permute(0, 3, 1, 2)
    assert float(pre.abs().max()) > 300.0
    neg = pre < -6.0
    assert bool(neg.any()) and float(y[neg].abs().max()) == 0.0, float(y[neg].abs().max())
    pos = pre > 6.0
    ref = pre.double().cpu()
    assert bool(((y.double().cpu() - ref)[pos.cpu()].abs() <= 8e-3 * ref[pos.cpu()].abs() + 1e-6).all())


@pytest.mark.parametrize("c", SHAPES)
def test_wide_channel_mlp_is_a_threshold(c):
    """Unsupported one token below M_min, and the raw entry refuses that call instead of launching."""
    from recnext_amd import _lib, ops
    m = _m_min(c) - 1
    assert m >= 1 and not ops.channel_mlp_supported(m, c, HID, torch.bfloat16) and not ops.channel_mlp_supported(m, c, 750, torch.bfloat16)
    assert ops.channel_mlp_supported(m + 1, c, 750, torch.bfloat16)
    assert not ops.channel_mlp_supported(1 << 20, c, HID, torch.float16) and not ops.channel_mlp_supported(1 << 20, c, HID, torch.float32)
    z = torch.zeros(1, c, 1, m, device=dev(), dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wfrag = torch.zeros(_lib.load().rcx_channel_mlp_pack_bytes(c, HID) // 2, device=dev(), dtype=torch.bfloat16)
    bias = torch.zeros(HID + c, device=dev())
    with pytest.raises(_lib.RcxError, match="no kernel"):
        ops.channel_mlp(z, z.clone(), wfrag, bias, HID)


def _count_fused(net, x):
    """(mixers whose forward took the fused launch, mixers in all, those of at most 256 channels, logits) in one forward of net on x."""
    from recnext_amd import models
    hits, handles = [0, 0, 0], []

    def hook(mod, inputs, output):
        fused = mod.__dict__.get("_fused_mlp")
        hits[1] += 1
        hits[2] += output.shape[1] <= 256
        if fused is not None and not mod.training and fused.supported(output):
            hits[0] += 1

    for m in net.modules():
        if isinstance(m, models._mlp_hosts()):
            handles.append(m.register_forward_hook(hook))
    with torch.no_grad():
        y = net(x)
    for hnd in handles:
        hnd.remove()
    return hits[0], hits[1], hits[2], y.float()


@pytest.mark.parametrize("name,mixers", [("recnext_t", 23), ("recnext_s", 23), ("recnext_m1", 26)])
def test_models_run_every_mixer_fused_above_m_min_and_the_library_below(name, mixers):
    """T: eleven (512, 768) mixers at 4 x 4; S: those and nine (384, 768) at 7 x 7; M1: three (384, 768) at 7 x 7.  (B's shapes are S's.)"""
    from recnext_amd.speed import build_inference_model, synthetic_batch
    a = build_inference_model(name, dev(), torch.bfloat16, seed=0, fused_mlp=False)
    b = build_inference_model(name, dev(), torch.bfloat16, seed=0, fused_mlp=True)
    batch = max(-(-_m_min(384) // 49), 1 if name == "recnext_m1" else -(-_m_min(512) // 16))
    x = synthetic_batch(batch, 224, dev(), torch.bfloat16, seed=1)
    fused, blocks, _, yb = _count_fused(b, x)
    assert (fused, blocks) == (mixers, mixers)
    with torch.no_grad():
        ya = a(x).float()
    scale = float(ya.abs().max())
    assert float((ya - yb).abs().max()) < 0.05 * scale + 0.02, (float((ya - yb).abs().max()), scale)
    assert 2 * 49 < _m_min(384) and 2 * 16 < _m_min(512)
    fused2, blocks2, narrow, _ = _count_fused(b, synthetic_batch(2, 224, dev(), torch.bfloat16, seed=1))
    assert blocks2 == mixers and 0 < narrow < mixers and fused2 == narrow            # batch 2: the new shapes keep the GEMM library
