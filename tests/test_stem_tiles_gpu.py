"""The fused stem's tiling, staging and store paths (rcx_stem.hip): planes that are not a multiple of the 8 x 8 output tile in either direction, a plane smaller than
one tile, widths whose rows (6 W bytes) are not a multiple of 4 / 8 / 16 (x staged as single bf16 instead of 8-byte pieces), an x that is only 2-byte aligned (a
sliced batch), more tiles than the persistent grid and fewer, output widths whose pixels are not 16-byte aligned (the 8-byte store path), and determinism over repeated
launches (the outputs pass through a per-wave LDS image).  Same float64 chain (intermediate rounded to bf16) and the same 1e-2 bar as tests/test_stem_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _reference(x, w1, b1, w2, b2):
    x64, w164, w264 = x.double().cpu(), w1.double().cpu(), w2.double().cpu()
    h = F.gelu(F.conv2d(x64, w164, b1.double().cpu(), stride=2, padding=1))
    h = h.to(torch.bfloat16).double()
    return F.conv2d(h, w264, b2.double().cpu(), stride=2, padding=1)


def _operands(n, cm, co, h, w, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    rb = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(torch.bfloat16).to(dev())
    x = rb(n, 3, h, w).contiguous(memory_format=torch.channels_last)
    return x, rb(cm, 3, 3, 3, sc=(2.0 / 27) ** 0.5), rb(cm, sc=0.3), rb(co, cm, 3, 3, sc=(2.0 / (9 * cm)) ** 0.5), rb(co, sc=0.3)


def _check(x, w1, b1, w2, b2, cm, co):
    from recnext_amd import ops
    n, _, h, w = x.shape
    assert ops.stem_supported(n, h, w, cm, co, torch.bfloat16)
    y = ops.stem(x, *ops.pack_stem(w1, b1, w2, b2), cm, co)
    ref = _reference(x, w1, b1, w2, b2)
    assert tuple(y.shape) == tuple(ref.shape)
    err = (y.double().cpu() - ref).abs()
    tol = 1e-2 + 1e-2 * ref.abs()
    print(f"\n{tuple(x.shape)} CM {cm} CO {co}: worst err / tol {float((err / tol).max()):.3f}, mean |err| {float(err.mean()):.2e}")
    assert bool(torch.isfinite(y).all())
    assert bool((err <= tol).all())
    return y


# (N, CM, CO, H, W)
CASES = [
    (2, 32, 64, 100, 76),      # 25 x 19 outputs: ragged tiles both ways; W % 4 == 0 (8-byte pieces)
    (1, 32, 64, 61, 90),       # W % 4 == 2: rows are a multiple of 4 bytes only
    (2, 24, 48, 45, 67),       # odd W: rows are a multiple of 2 bytes only; odd image size
    (1, 20, 40, 30, 52),       # W % 8 == 4: rows a multiple of 8, not of 16
    (3, 32, 64, 13, 9),        # a plane smaller than one tile (4 x 3 outputs)
    (1, 28, 44, 40, 40),       # CO % 8 == 4: a pixel of y is 8-byte aligned only
    (1, 40, 80, 72, 200),      # KC = 48, three output tiles, one workgroup per compute unit
    (1, 32, 96, 36, 36),       # CO = 96
    (5, 32, 64, 3, 5),         # 1 x 2 outputs
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_stem_tiles_and_staging_paths(case):
    n, cm, co, h, w = case
    _check(*_operands(n, cm, co, h, w, seed=7 * h + w), cm, co)


@pytest.mark.parametrize("case", [(3, 32, 64, 33, 36), (3, 24, 48, 35, 35), (4, 32, 64, 32, 64)], ids=lambda c: "x".join(map(str, c)))
def test_stem_on_a_sliced_batch(case):
    """x[1:] of a channels_last batch starts H W 6 bytes into the allocation: 2-byte aligned for an odd plane, 8-byte for an even one."""
    n, cm, co, h, w = case
    x, w1, b1, w2, b2 = _operands(n, cm, co, h, w, seed=11)
    xs = x[1:]
    assert xs.is_contiguous(memory_format=torch.channels_last)
    y = _check(xs, w1, b1, w2, b2, cm, co)
    from recnext_amd import ops
    whole = ops.stem(x, *ops.pack_stem(w1, b1, w2, b2), cm, co)
    assert torch.equal(y, whole[1:]), "an image's output depends on where the batch starts"


def test_stem_more_tiles_than_the_grid_and_fewer():
    """One tile, and several tiles per persistent workgroup (more than 2 x 256 x 2 tiles), whole-batch result equal to the per-image results."""
    from recnext_amd import ops
    x, w1, b1, w2, b2 = _operands(1, 32, 64, 32, 32, seed=3)
    _check(x, w1, b1, w2, b2, 32, 64)                                      # 1 tile
    x, w1, b1, w2, b2 = _operands(12, 32, 64, 224, 224, seed=5)            # 12 x 49 = 588 tiles: above a grid of 2 x 256, below 2 per workgroup
    y = _check(x[:2], w1, b1, w2, b2, 32, 64)
    pack = ops.pack_stem(w1, b1, w2, b2)
    whole = ops.stem(x, *pack, 32, 64)
    assert torch.equal(whole[:2], y)
    x2 = torch.cat([x] * 4)                                                # 2 352 tiles: four to five per workgroup
    assert torch.equal(ops.stem(x2, *pack, 32, 64), torch.cat([whole] * 4))


@pytest.mark.parametrize("case", [(8, 32, 64, 224, 224), (2, 24, 48, 45, 67), (1, 40, 80, 72, 200)], ids=lambda c: "x".join(map(str, c)))
def test_stem_is_deterministic_over_40_launches(case):
    from recnext_amd import ops
    n, cm, co, h, w = case
    x, w1, b1, w2, b2 = _operands(n, cm, co, h, w, seed=13)
    pack = ops.pack_stem(w1, b1, w2, b2)
    first = ops.stem(x, *pack, cm, co)
    for _ in range(40):
        assert torch.equal(ops.stem(x, *pack, cm, co), first)
