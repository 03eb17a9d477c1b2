"""The software-pipelined phase A of the one-launch stem (rcx_stem.hip: biases in registers, the GELU of a pixel tile in lockstep under the next pixel tile's gather
and products, the shared last round of pixel tiles) -- every case is one in which only a new code path can go wrong:

  * one 8 x 8 output tile: all ten pixel tiles of the 17 x 17 intermediate and the last round run, nothing else;
  * more tiles than the persistent grid (2 x compute units), so that workgroups walk two and three tiles: the pipeline's hand-over between tiles and the
    biases held in registers across the tile loop;
  * planes whose 17 x 17 intermediate crosses every border of its plane (the `inside` zeros; odd widths take the 2-byte x path);
  * a sliced batch that starts on an odd plane (x 2-byte aligned), with CO % 8 == 4 as well so that y leaves by the 8-byte store path;
  * channels past CM (20, 24, 28) and CM = 40 / CO = 80 (two tiles of the first product, KC = 48, three output tiles, one workgroup per compute unit);
  * the GELU in the output epilogue (the front launch of the T / S / B stem) through ops.stem3 at (CM, CO) = (16, 32) and (32, 64).

Each case: the float64 chain of tests/test_stem_gpu.py (tests/test_ls_stem_gpu.py's for stem3) with the intermediates rounded to bf16, at that file's bar
1e-2 + 1e-2 |ref| on every element; torch.equal over 40 repeated launches; and the sha256 of the output bytes equal to what the parent's kernel wrote
(tests/golden/stem_parent_bits.json, recorded by tests/golden/make_golden_stem_bits.py on the parent commit's build): the rework changes no float32 operation,
operand or summation order, so the outputs are bit-identical."""
import functools
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stem_parent_bits.json")

# id -> (kind, N, CM, CO, H, W, first image of the slice, seed of the CPU generator); stem3: C = 2 CO, final GELU on
CASES = {
    "one-tile-3x32x64x32x32": ("stem", 3, 32, 64, 32, 32, 0, 101),
    "walk-48x32x64x160x160": ("stem", 48, 32, 64, 160, 160, 0, 102),          # 48 x 25 = 1200 tiles > 2 x 256: two and three tiles a workgroup
    "border-1x1": ("stem", 2, 32, 64, 1, 1, 0, 103),
    "border-2x2": ("stem", 2, 32, 64, 2, 2, 0, 104),
    "border-17x16": ("stem", 1, 32, 64, 17, 16, 0, 105),
    "border-37x51": ("stem", 2, 32, 64, 37, 51, 0, 106),
    "sliced-odd-plane-32x64": ("stem", 3, 32, 64, 33, 35, 1, 107),            # x[1:] starts 6930 bytes in: 2-byte aligned
    "sliced-odd-plane-28x44": ("stem", 3, 28, 44, 33, 35, 1, 108),            # ... and CO % 8 == 4: the 8-byte store path
    "cm20-40x24": ("stem", 2, 20, 40, 40, 24, 0, 109),
    "cm24-40x24": ("stem", 2, 24, 48, 40, 24, 0, 110),
    "cm28-40x24": ("stem", 2, 28, 56, 40, 24, 0, 111),
    "cm40-co80-40x24": ("stem", 2, 40, 80, 40, 24, 0, 112),
    "go-16x32-40x24": ("stem3", 2, 16, 32, 40, 24, 0, 113),
    "go-32x64-40x24": ("stem3", 2, 32, 64, 40, 24, 0, 114),
}


def dev():
    return torch.device("cuda:0")


def output_sha256(y):
    """sha256 of y's bytes in storage (N x H x W x C) order."""
    return hashlib.sha256(y.permute(0, 2, 3, 1).contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def make_case(name):
    """-> (launch, reference): launch() runs the kernel(s) once more on the case's operands, reference() is the float64 chain on the same operands."""
    from recnext_amd import ops
    kind, n, cm, co, h, w, first, seed = CASES[name]
    if kind == "stem":
        from tests.test_stem_gpu import _reference
        g = torch.Generator(device="cpu").manual_seed(seed)
        rb = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(torch.bfloat16).to(dev())
        x = rb(n, 3, h, w).contiguous(memory_format=torch.channels_last)[first:]
        w1, b1, w2, b2 = rb(cm, 3, 3, 3, sc=(2.0 / 27) ** 0.5), rb(cm, sc=0.3), rb(co, cm, 3, 3, sc=(2.0 / (9 * cm)) ** 0.5), rb(co, sc=0.3)
        assert x.is_contiguous(memory_format=torch.channels_last) and ops.stem_supported(x.shape[0], h, w, cm, co, torch.bfloat16)
        pack = ops.pack_stem(w1, b1, w2, b2)
        return (lambda: ops.stem(x, *pack, cm, co)), (lambda: _reference(x, w1, b1, w2, b2))
    from tests.test_ls_stem_gpu import _operands, _reference
    x, ws = _operands(n, 2 * co, h, w, seed=seed)
    assert ops.stem3_supported(n, h, w, 2 * co, True, torch.bfloat16)
    pack = ops.pack_stem3(*ws)
    return (lambda: ops.stem3(x, *pack, 2 * co, True)), (lambda: _reference(x, ws, True))


@functools.lru_cache(maxsize=None)
def _ran(name):
    """The case's launcher, its first output and the float64 reference: computed once, shared by the tests below, never modified."""
    launch, reference = make_case(name)
    return launch, launch(), reference()


@pytest.mark.parametrize("name", list(CASES))
def test_stem_pipeline_against_float64_and_over_40_launches(name):
    launch, y, ref = _ran(name)
    assert tuple(y.shape) == tuple(ref.shape) and y.dtype == torch.bfloat16
    err = (y.double().cpu() - ref).abs()
    tol = 1e-2 + 1e-2 * ref.abs()                         # tests/test_stem_gpu.py's bar, every element
    print(f"\n{name}: worst err / tol {float((err / tol).max()):.3f}, mean |err| {float(err.mean()):.2e}")
    assert bool(torch.isfinite(y).all())
    assert bool((err <= tol).all())
    for _ in range(40):
        assert torch.equal(launch(), y), "not deterministic"


@pytest.mark.parametrize("name", list(CASES))
def test_stem_output_bits_are_the_parents(name):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(CASES)
    assert golden[name]["seed"] == CASES[name][-1]
    _, y, _ = _ran(name)
    assert output_sha256(y) == golden[name]["sha256"], "the output is not bit-identical to the parent kernel's"
