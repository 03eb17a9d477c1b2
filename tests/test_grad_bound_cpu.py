"""CPU: the per-element float64 bound of tests/grad64.py accepts correctly rounded gradients and rejects the kinds of error a flat
1e-2 x max|ref| bar lets through; and the backward entry points of recnext_amd.ops refuse mismatched extents before any launch."""
import pytest
import torch

from tests import grad64
from tests.grad64 import U32, assert_grad_close

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _synthetic(seed=0, shape=(2, 8, 14, 14)):
    """A float64 'gradient' that is the sum of 64 products per element, and M, the sum of their magnitudes.  The border rows and columns are
    scaled down to about 1e-3 of the interior, as a border gradient of a padded conv can be."""
    g = torch.Generator().manual_seed(seed)
    terms = torch.randn((64,) + shape, generator=g, dtype=torch.float64) * torch.randn((64,) + shape, generator=g, dtype=torch.float64)
    scale = torch.ones(shape, dtype=torch.float64)
    scale[..., 0, :] = scale[..., -1, :] = 1e-3
    scale[..., :, 0] = scale[..., :, -1] = 1e-3
    terms = terms * scale
    return terms.sum(0), terms.abs().sum(0)


def _rtz(ref, dtype):
    """Round toward zero to dtype (by rounding to nearest, then stepping one ulp toward zero where that went away from zero)."""
    r = ref.to(dtype)
    away = r.double().abs() > ref.abs()
    toward = torch.nextafter(r.float(), torch.zeros_like(r.float())).to(dtype) if dtype == torch.float32 else _step_toward_zero(r)
    return torch.where(away, toward, r)


def _step_toward_zero(r):
    bits = r.view(torch.int16)
    return torch.where(r != 0, bits - 1, bits).view(r.dtype)        # sign-magnitude: one less in the magnitude bits is one ulp toward zero


def _step_away(r):
    return (r.view(torch.int16) + 1).view(r.dtype) if r.dtype != torch.float32 else torch.nextafter(r, r * 2)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_correctly_rounded_values_pass(dtype):
    ref, mag = _synthetic()
    assert assert_grad_close(ref.to(dtype), ref, mag, dtype) <= 1.0
    # ... and so do values carrying a float32 accumulation error well inside K u32 M before the final rounding
    noisy = (ref + (grad64.K / 2) * U32 * mag * torch.sign(torch.randn_like(ref))).to(torch.float32).to(dtype)
    assert_grad_close(noisy, ref, mag, dtype)


def test_subnormal_and_zero_outputs_pass():
    ref = torch.tensor([0.0, 1e-42, -3e-7, 2.0 ** -140], dtype=torch.float64)
    mag = ref.abs()
    for dtype in DTYPES:
        assert_grad_close(ref.to(dtype), ref, mag, dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=str)
def test_round_toward_zero_is_rejected(dtype):
    ref, mag = _synthetic(1)
    got = _rtz(ref, dtype)
    assert bool((got.double() != ref.to(dtype).double()).any())
    with pytest.raises(AssertionError, match="outside the bound"):
        assert_grad_close(got, ref, mag, dtype)
    # a flat bar of 1e-2 x max|ref| does not see it
    assert float((got.double() - ref).abs().max()) < 1e-2 * float(ref.abs().max())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=str)
def test_one_ulp_bias_on_one_percent_is_rejected(dtype):
    ref, mag = _synthetic(2)
    got = ref.to(dtype)
    pick = torch.rand(ref.shape, generator=torch.Generator().manual_seed(3)) < 0.01
    assert int(pick.sum()) > 0
    got = torch.where(pick, _step_away(got), got)
    with pytest.raises(AssertionError, match="outside the bound"):
        assert_grad_close(got, ref, mag, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("edge", ["row", "col"])
def test_border_line_off_by_five_percent_is_rejected(dtype, edge):
    ref, mag = _synthetic(4)
    bad = ref.clone()
    if edge == "row":
        bad[1, 3, -1, :] *= 1.05
    else:
        bad[0, 5, :, 0] *= 1.05
    got = bad.to(dtype)
    with pytest.raises(AssertionError, match=r"worst at \(n=\d+, c=\d+, h=\d+, w=\d+\)") as e:
        assert_grad_close(got, ref, mag, dtype)
    where = (1, 3, ref.shape[2] - 1) if edge == "row" else (0, 5)
    assert "n=%d, c=%d" % where[:2] in str(e.value)
    assert float((got.double() - ref).abs().max()) < 1e-2 * float(ref.abs().max())        # far below the plane maximum


def test_dropped_float32_term_is_rejected():
    ref, mag = _synthetic(5)
    got = ref.clone()
    got[0, 2, 7, 7] -= 100 * U32 * mag[0, 2, 7, 7]
    got = got.to(torch.float32)
    with pytest.raises(AssertionError, match=r"worst at \(n=0, c=2, h=7, w=7\)"):
        assert_grad_close(got, ref, mag, torch.float32)


def test_ulp16_matches_the_formats():
    a = torch.tensor([1.0, 1.5, 2.0 ** -20, 0.0, 65504.0], dtype=torch.float64)
    assert grad64.ulp16(a, torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -27, 2.0 ** -133, 2.0 ** 8]
    assert grad64.ulp16(a, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -24, 2.0 ** -24, 32.0]
    for dtype in (torch.bfloat16, torch.float16):
        x = torch.tensor([1.0, 3.0, 1000.0], dtype=dtype)
        nxt = (x.view(torch.int16) + 1).view(dtype)
        assert torch.equal((nxt.double() - x.double()), grad64.ulp16(x.double(), dtype))


# ---- argument checks of the backward entry points (recnext_amd/ops.py): run on CPU tensors, before the library is called ----

def _nhwc(*shape):
    return torch.zeros(shape).contiguous(memory_format=torch.channels_last)


def _gpu_refusal():
    from recnext_amd import _lib
    return pytest.raises(_lib.RcxError, match="on cpu")


def test_dwconv2d_backward_checks_extents():
    from recnext_amd import ops
    x, w = _nhwc(2, 8, 14, 14), torch.zeros(25 * 8)
    for gy in (_nhwc(2, 8, 14, 14), _nhwc(2, 8, 7, 6), _nhwc(1, 8, 7, 7), _nhwc(2, 4, 7, 7)):
        with pytest.raises(ValueError, match="gy"):
            ops.dwconv2d_backward(x, gy, w, 5, 2)
    with pytest.raises(ValueError, match="w_kkc"):
        ops.dwconv2d_backward(x, _nhwc(2, 8, 7, 7), torch.zeros(25 * 4), 5, 2)
    with pytest.raises(ValueError, match="gy"):
        ops.dwconv2d_backward(x, _nhwc(2, 8, 7, 7), w, 5, 1)
    with pytest.raises(ValueError, match="gy"):
        ops.dwconv2d_backward(x, torch.zeros(2, 8, 7, 7, device="meta"), w, 5, 2)
    with _gpu_refusal():
        ops.dwconv2d_backward(x, _nhwc(2, 8, 7, 7), w, 5, 2)
    with _gpu_refusal():
        ops.dwconv2d_backward(x, _nhwc(2, 8, 14, 14), w, 5, 1)


def test_dwconv2d_mult2_backward_checks_extents():
    from recnext_amd import ops
    x, w = _nhwc(2, 8, 14, 14), torch.zeros(49 * 16)
    for gy in (_nhwc(2, 8, 7, 7), _nhwc(2, 16, 14, 14), _nhwc(3, 16, 7, 7)):
        with pytest.raises(ValueError, match="gy"):
            ops.dwconv2d_mult2_backward(x, gy, w, 7)
    with pytest.raises(ValueError, match="w_kkc"):
        ops.dwconv2d_mult2_backward(x, _nhwc(2, 16, 7, 7), torch.zeros(49 * 8), 7)
    with _gpu_refusal():
        ops.dwconv2d_mult2_backward(x, _nhwc(2, 16, 7, 7), w, 7)


def test_upadd_dwconv_backward_checks_extents():
    from recnext_amd import ops
    x, c, gy, w = _nhwc(2, 8, 14, 14), _nhwc(2, 8, 7, 7), _nhwc(2, 8, 14, 14), torch.zeros(25 * 8)
    for bad in (_nhwc(1, 8, 7, 7), _nhwc(2, 4, 7, 7)):
        with pytest.raises(ValueError, match="coarse"):
            ops.upadd_dwconv_backward(x, bad, gy, w)
    for bad in (_nhwc(2, 8, 7, 7), _nhwc(2, 8, 14, 13), _nhwc(2, 12, 14, 14)):
        with pytest.raises(ValueError, match="gy"):
            ops.upadd_dwconv_backward(x, c, bad, w)
    with pytest.raises(ValueError, match="w_kkc"):
        ops.upadd_dwconv_backward(x, c, gy, torch.zeros(9 * 8))
    with pytest.raises(ValueError, match="coarse"):
        ops.upadd_dwconv_backward(x, torch.zeros(2, 8, 7, 7, device="meta"), gy, w)
    with _gpu_refusal():
        ops.upadd_dwconv_backward(x, c, gy, w)


def test_recconv2d_backward_checks_extents():
    from recnext_amd import ops
    c, k, level = 8, 5, 2
    x, gy, wpack, saved = _nhwc(2, c, 14, 14), _nhwc(2, c, 14, 14), torch.zeros(4 * k * k * c), torch.zeros(1 << 20, dtype=torch.uint8)
    for bad in (_nhwc(2, c, 14, 7), _nhwc(1, c, 14, 14), _nhwc(2, 4, 14, 14)):
        with pytest.raises(ValueError, match="gy"):
            ops.recconv2d_backward(x, bad, wpack, saved, level, k)
    with pytest.raises(ValueError, match="wpack"):
        ops.recconv2d_backward(x, gy, torch.zeros(3 * k * k * c), saved, level, k)
    with pytest.raises(ValueError, match="wflip"):
        ops.recconv2d_backward(x, gy, wpack, saved, level, k, wflip=torch.zeros(2 * k * k * c))
    with pytest.raises(ValueError, match="saved"):
        ops.recconv2d_backward(x, gy, wpack, torch.zeros(16, dtype=torch.uint8, device="meta"), level, k)
    with _gpu_refusal():
        ops.recconv2d_backward(x, gy, wpack, saved, level, k, wflip=wpack.clone())


def test_recconv2d_backward_checks_the_saved_size():
    """The size of the saved pyramid comes from the library's size query (host code: no GPU needed, but the built library is)."""
    from recnext_amd import _lib, ops
    import os
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("the library is not built (run __graft_entry__.build())")
    lib = _lib.load()
    x = torch.zeros(2, 8, 14, 14, device="meta")
    need = lib.rcx_recconv2d_train_saved_bytes(2, 8, 14, 14, 2, 5)
    assert need > 0
    with pytest.raises(ValueError, match="saved"):
        ops.recconv2d_backward(x, x, torch.zeros(4 * 25 * 8, device="meta"), torch.zeros(need - 1, dtype=torch.uint8, device="meta"), 2, 5)
