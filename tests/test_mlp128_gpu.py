"""The 128-channel channel mixer on LDS-resident weights (rcx_mlp.hip k_channel_mlp_res128: C = 128, hidden <= 256, every token count): free-running waves,
each walking its own 32-token tiles, one barrier after the prologue.  Against the float64 formula and the library chain with the assertions of
test_mlp_gpu.py::test_fused_channel_mlp_against_float64_and_the_gemm_path, at the shapes where this form can go wrong: waves without a tile, fewer tiles than
waves, ragged last tiles, several workgroups, a padded hidden layer, and more tiles than the grid has wave slots (waves that loop)."""
import functools

import pytest
import torch

from tests import guard
from tests.mlp_common import check, dev, operands, reference

pytestmark = pytest.mark.gpu

C = 128
NW = 8                                                   # waves of a workgroup; one persistent workgroup per compute unit


def _looping_case():
    """(21, 256, 56, 57) on 256 compute units: 2 094.75 tiles on 2 048 wave slots -- some waves take two tiles, some one, the last tile is ragged.  N grows
    with the device so that M > 32 * 8 * (compute units) holds rather than being assumed."""
    cus = torch.cuda.get_device_properties(dev()).multi_processor_count
    n = 21
    while n * 56 * 57 <= 32 * NW * cus:
        n += 1
    assert n * 56 * 57 > 32 * NW * cus and (n * 56 * 57) % 32
    return (n, 256, 56, 57)


SMALL = {"1x1": (1, 256, 1, 1), "3x5": (1, 256, 3, 5), "9x11": (1, 256, 9, 11), "3x28x28": (3, 256, 28, 28), "hidden240": (1, 240, 3, 33)}
RAGGED = ("1x1", "3x5", "9x11", "3x28x28", "hidden240", "looping")


def _case(which):
    return _looping_case() if which == "looping" else SMALL[which]


@functools.lru_cache(maxsize=None)
def _operands(which):
    """The case's operands, pack and plain result: made once, shared by the tests, never modified."""
    from recnext_amd import ops
    n, hid, h, w = _case(which)
    z, x, w1, b1, w2, b2 = operands(n, C, hid, h, w, seed=C * 1000 + hid + h + 7 * w)
    hp = ops.channel_mlp_hidden(n * h * w, C, hid, torch.bfloat16)
    assert hp == 256                                     # 240 is padded with zero units
    wfrag, bias, hp2 = ops.pack_channel_mlp(w1, b1, w2, b2, hidden_to=hp)
    assert hp2 == hp
    y = ops.channel_mlp(z, x, wfrag, bias, hp)
    return z, x, w1, b1, w2, b2, wfrag, bias, hp, y


@pytest.mark.parametrize("which", RAGGED)
def test_resident_channel_mlp_against_float64_and_the_gemm_path(which):
    from recnext_amd import ops
    n, hid, h, w = _case(which)
    z, x, w1, b1, w2, b2, wfrag, bias, hp, y = _operands(which)
    assert y.shape == x.shape and y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, ops.channel_mlp(z, x, wfrag, bias, hp)), "not deterministic"
    ref = reference(z, x, w1, b1, w2, b2)
    err = check(y, ref, (n, C, hid, h, w))
    zz = z.permute(0, 2, 3, 1).reshape(-1, C)
    lib = torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(zz, w1, b1)), w2, b2)
    lib = x + lib.view(n, h, w, C).permute(0, 3, 1, 2)
    lib_err = (lib.double().cpu() - ref).abs()
    print(f"    mean |err| fused {float(err.mean()):.2e} / library {float(lib_err.mean()):.2e}; max {float(err.max()):.2e} / {float(lib_err.max()):.2e}")
    assert float(err.mean()) <= 1.05 * float(lib_err.mean()) and float(err.max()) <= 1.25 * float(lib_err.max()) + 1e-3


@pytest.mark.parametrize("which", RAGGED)
def test_resident_channel_mlp_stays_inside_its_tensors(which):
    """z, x and y each inside a larger buffer with sentinel margins (tests/guard.py): y's margins are untouched, every element of y is written, and the result
    does not depend on what the margins of z and x hold -- at every ragged case, the looping one included."""
    from recnext_amd import ops
    z, x, _, _, _, _, wfrag, bias, hp, y = _operands(which)
    got = guard.run_properties(lambda z, x, wfrag, bias: ops.channel_mlp(z, x, wfrag, bias, hp), (z, x, wfrag, bias), repeat=False)
    assert torch.equal(got, y)


@pytest.mark.parametrize("which", ["9x11", "looping"])
def test_resident_channel_mlp_repeated_launches_give_equal_bits(which):
    """The free-running waves share the resident pack and nothing else: 40 launches, equal bits every time (a missing hand-off around a wave's image shows here)."""
    from recnext_amd import ops
    z, x, _, _, _, _, wfrag, bias, hp, y = _operands(which)
    outs = [ops.channel_mlp(z, x, wfrag, bias, hp) for _ in range(40)]
    same = torch.stack([(o == y).all() for o in outs]).cpu().tolist()      # one read-back
    assert all(same), f"launches that differ: {[i for i, s in enumerate(same) if not s]}"


@pytest.mark.parametrize("name", ["recnext_m3", "recnext_a3"])
def test_model_with_the_resident_mixer_matches_the_gemm_path(name):
    """M3 and A3 at batch 2 through models.use_fused_mlp (the 28 x 28 stage and its Downsample mixer; A3's hidden 240 padded to 256) against the library path,
    within the model bar of test_mlp_gpu.py."""
    from recnext_amd import models
    from recnext_amd.speed import build_inference_model, synthetic_batch
    a = build_inference_model(name, dev(), torch.bfloat16, seed=0, fused_mlp=False)
    b = build_inference_model(name, dev(), torch.bfloat16, seed=0, fused_mlp=True)
    hosts = [m for m in b.modules() if m.__dict__.get("_fused_mlp") is not None and isinstance(m, (models.MetaNeXtBlock, models.Downsample))]
    t = torch.empty(2, C, 28, 28, device=dev(), dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    at128 = [m for m in hosts if m.channel_mixer[0].in_channels == C and m._fused_mlp.supported(t)]
    assert len(at128) >= models.CONFIGS[name]["depth"][1]                  # the fused launch is what runs at 128 channels
    x = synthetic_batch(2, 224, dev(), torch.bfloat16, seed=1)
    with torch.no_grad():
        ya, yb = a(x).float(), b(x).float()
    scale = float(ya.abs().max())
    print(f"\n{name}: max |diff| {float((ya - yb).abs().max()):.4f} at scale {scale:.3f}")
    assert float((ya - yb).abs().max()) < 0.05 * scale + 0.02, (float((ya - yb).abs().max()), scale)
