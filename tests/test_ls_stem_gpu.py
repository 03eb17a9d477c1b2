"""The T / S / B stem on HIP (rcx_stem3_fwd: conv1 + GELU + conv2 + GELU in one launch, conv3 (+ GELU) in a second; ops.stem3, layers.FusedStem3,
lsmodels.RecNextStem after models.use_fused_stem) against the float64 chain on the same bf16 operands with both intermediates rounded to bf16 (what the
library path and the kernels both do), and against the library path itself.  Reference: lsnet/model/recattn.py:208-223."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import guard

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _operands(n, c, h, w, seed=None):
    """As tests/test_stem_gpu.py: weights scaled sqrt(2 / (9 Cin)), biases 0.3, everything rounded to bf16."""
    g = torch.Generator(device="cpu").manual_seed(c * 100 + h if seed is None else seed)
    rb = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(torch.bfloat16).to(dev())
    x = rb(n, 3, h, w).contiguous(memory_format=torch.channels_last)
    ws = []
    for cin, cout in ((3, c // 4), (c // 4, c // 2), (c // 2, c)):
        ws += [rb(cout, cin, 3, 3, sc=(2.0 / (9 * cin)) ** 0.5), rb(cout, sc=0.3)]
    return x, ws


def _reference(x, ws, act):
    """tests/test_stem_gpu.py::_reference extended by one conv: float64 sums, each intermediate a bf16 tensor."""
    w1, b1, w2, b2, w3, b3 = (t.double().cpu() for t in ws)
    h = F.gelu(F.conv2d(x.double().cpu(), w1, b1, stride=2, padding=1)).to(torch.bfloat16).double()
    h = F.gelu(F.conv2d(h, w2, b2, stride=2, padding=1)).to(torch.bfloat16).double()
    y = F.conv2d(h, w3, b3, stride=2, padding=1)
    return F.gelu(y) if act else y


def _library(x, ws, act):
    w1, b1, w2, b2, w3, b3 = ws
    y = F.conv2d(F.gelu(F.conv2d(F.gelu(F.conv2d(x, w1, b1, stride=2, padding=1)), w2, b2, stride=2, padding=1)), w3, b3, stride=2, padding=1)
    return F.gelu(y) if act else y


def _down3(v):
    for _ in range(3):
        v = -(-v // 2)
    return v


CASES = [(2, 128, 224, 224, False), (2, 64, 224, 224, True), (1, 128, 64, 96, True), (1, 64, 37, 51, True), (1, 128, 9, 23, True), (3, 128, 8, 8, False),
         (1, 128, 1, 1, True), (1, 64, 17, 16, False), (1, 128, 256, 320, False), (2, 64, 130, 66, False)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, map(int, c))))
def test_stem3_against_float64_and_the_conv_library(case):
    from recnext_amd import ops
    n, c, h, w, act = case
    x, ws = _operands(n, c, h, w)
    assert ops.stem3_supported(n, h, w, c, act, torch.bfloat16)
    pack = ops.pack_stem3(*ws)
    y = ops.stem3(x, *pack, c, act)
    assert tuple(y.shape) == (n, c, _down3(h), _down3(w)) and y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    ref = _reference(x, ws, act)
    err = (y.double().cpu() - ref).abs()
    tol = 1e-2 + 1e-2 * ref.abs()                         # the project's bf16 bar
    lib_err = (_library(x, ws, act).double().cpu() - ref).abs()
    print(f"\n{case}: worst err / tol {float((err / tol).max()):.3f}; mean |err| HIP {float(err.mean()):.2e} / library {float(lib_err.mean()):.2e}")
    assert bool((err <= tol).all())
    assert float(err.mean()) <= 1.05 * float(lib_err.mean()) + 1e-5


@pytest.mark.parametrize("c,h,w", [(64, 37, 51), (128, 64, 96)])
def test_stem3_is_deterministic_and_batch_independent(c, h, w):
    from recnext_amd import ops
    x, ws = _operands(3, c, h, w)
    pack = ops.pack_stem3(*ws)
    y = ops.stem3(x, *pack, c, True)
    assert torch.equal(y, ops.stem3(x, *pack, c, True)), "not deterministic"
    one = ops.stem3(x[1:2], *pack, c, True)               # (an odd plane: a base that is no multiple of 8 bytes)
    assert torch.equal(one, y[1:2])


def test_stem3_refuses_what_it_has_no_kernel_for():
    from recnext_amd import ops
    assert ops.stem3_supported(1, 224, 224, 64, True, torch.bfloat16) and ops.stem3_supported(256, 224, 224, 128, False, torch.bfloat16)
    assert not ops.stem3_supported(1, 224, 224, 128, True, torch.float32) and not ops.stem3_supported(1, 224, 224, 128, True, torch.float16)
    for c in (32, 96, 256):
        assert not ops.stem3_supported(1, 224, 224, c, True, torch.bfloat16)
    x, ws = _operands(1, 64, 16, 16)
    pack = ops.pack_stem3(*ws)
    with pytest.raises(ValueError):
        ops.stem3(x, *pack, 96, True)                                        # a channel count without a kernel
    with pytest.raises(ValueError):
        ops.stem3(x, *pack, 128, True)                                       # packs of another channel count
    with pytest.raises(ValueError):
        ops.stem3(x, *pack[:4], pack[4][:-512], pack[5], 64, True)           # a short pack
    with pytest.raises(ValueError):
        ops.stem3(x.contiguous(), *pack, 64, True)                           # not channels_last
    with pytest.raises(ValueError):
        ops.stem3(torch.cat([x, x], 1).contiguous(memory_format=torch.channels_last), *pack, 64, True)      # six input channels
    with pytest.raises(ValueError):
        ops.pack_stem3(ws[0], ws[1], ws[2], ws[3], ws[4][:, :-1], ws[5])
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,c,h,w,sliced", [(1, 64, 37, 51, False), (3, 128, 37, 51, True), (3, 128, 8, 8, False)], ids=["64-37x51", "128-37x51-sliced", "128-8x8"])
def test_stem3_guard_bands(n, c, h, w, sliced):
    """tests/guard.py properties A - E: nothing outside an allocation written, every output element written, nothing outside an input read, inputs left alone,
    and the workspace exactly as large as its query says."""
    from recnext_amd import _lib, ops
    x, ws = _operands(n, c, h, w)
    if sliced:
        x = x[1:]
    pack = ops.pack_stem3(*ws)
    lib = _lib.load()

    def invoke(x_, *p):
        return ops.stem3(x_, *p, c, True)

    mods = guard.LIBRARY_MODULES + ("recnext_amd.lsstem",)                     # the workspace is that module's own torch.empty
    with guard.guarded_library(mods) as rec:
        invoke(x, *pack)
        torch.cuda.synchronize()
        sizes = [(a.tensor.dtype, a.nbytes) for a in rec.arenas]
    assert (torch.uint8, lib.rcx_stem3_workspace_bytes(x.shape[0], h, w, c)) in sizes and len(sizes) == 2, sizes       # E: the workspace is its query, to the byte
    guard.run_properties(invoke, (x,) + tuple(pack), modules=mods)


@pytest.mark.parametrize("name", ["recnext_t", "recnext_b", "recnext_s_share_channel"])
def test_model_with_the_hip_stem_matches_the_conv_library(name):
    from recnext_amd.layers import FusedStem3
    from recnext_amd.speed import build_inference_model, synthetic_batch
    a = build_inference_model(name, dev(), torch.bfloat16, seed=0, fused_stem=False)
    b = build_inference_model(name, dev(), torch.bfloat16, seed=0, fused_stem=True)
    assert list(a.state_dict()) == list(b.state_dict())
    assert isinstance(b.stem.__dict__.get("_fused_stem"), FusedStem3) and a.stem.__dict__.get("_fused_stem") is None
    x = synthetic_batch(4, 224, dev(), torch.bfloat16, seed=1)
    assert b.stem._fused_stem.supported(x)
    with torch.no_grad():
        assert b.stem._fused_stem.usable(b.stem.stem, x)
        sa, sb = a.stem(x).float(), b.stem(x).float()
        ya, yb = a(x).float(), b(x).float()
    assert len(b.stem._fused_stem.packs()) == 6                               # the HIP path ran
    assert float((sa - sb).abs().max()) < 0.02 * float(sa.abs().max()) + 0.02
    scale = float(ya.abs().max())
    assert float((ya - yb).abs().max()) < 0.05 * scale + 0.02, (float((ya - yb).abs().max()), scale)
    # a gradient wanted, then a replaced activation: the library path, bit for bit what the unfused model computes
    xg = x.clone().requires_grad_()
    assert not b.stem._fused_stem.usable(b.stem.stem, xg)
    assert torch.equal(b.stem(xg).detach(), a.stem(x).detach())
    b.stem.stem[1] = nn.ReLU()
    a.stem.stem[1] = nn.ReLU()
    with torch.no_grad():
        assert not b.stem._fused_stem.usable(b.stem.stem, x)
        assert torch.equal(b.stem(x), a.stem(x))


def test_graph_replay_of_recnext_t_follows_a_stem_weight_change():
    from recnext_amd.graph import GraphedInference
    from recnext_amd.speed import build_inference_model, synthetic_batch
    net = build_inference_model("recnext_t", dev(), torch.bfloat16, seed=0)
    run = GraphedInference(net)
    x = synthetic_batch(2, 224, dev(), torch.bfloat16, seed=0)
    with torch.no_grad():
        want = net(x).clone()
        assert len(net.stem._fused_stem.packs()) == 6
        assert torch.equal(run(x), want)
        net.stem.stem[0].weight.mul_(1.5)                                    # in place: the packs are rebuilt, the graph captured again
        want2 = net(x).clone()
        assert not torch.equal(want2, want)
        assert torch.equal(run(x), want2)
    assert len(run._graphs) == 1
