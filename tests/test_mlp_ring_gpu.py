"""The hidden step of the channel mixer's ring kernels (rcx_mlp.hip: mlp::hidden_tile_ring and its pinned form hidden_tile_pinned) through each of its four
callers -- k_channel_mlp (C = 64), k_channel_mlp_stream (C = 192), k_channel_mlp_pair (C = 256), k_channel_mlp_res128 (C = 128) -- at the smallest shapes at
which a step can go wrong: one token, a full tile and a one-token tile, one token past a workgroup's block, a workgroup that loops over more blocks than the grid
has, a padded hidden width, the aliased call (z is x) and 40 repeated launches.  Every result is checked against the float64 formula on the same bf16 operands
at test_mlp_gpu.py's bar; the pinned form keeps hidden_tile_ring's float32 operations and their order, so that bar's margins hold."""
import functools

import pytest
import torch

from tests.mlp_common import check, dev, operands, reference

pytestmark = pytest.mark.gpu

# caller -> (C, hidden, padded-from hidden, tokens of a workgroup's block)
KERNELS = {"small64": (64, 128, 120, 384), "stream192": (192, 384, 360, 128), "pair256": (256, 512, 480, 256), "res128": (128, 256, 240, 256)}
CASES = ("one", "tile_and_one", "block_and_one", "looping", "padded")


def _plane(kernel, case):
    """(N, H, W, hidden) of the case: M = N H W tokens"""
    c, hid, hid_from, block = KERNELS[kernel]
    if case == "one":
        return 1, 1, 1, hid
    if case == "tile_and_one":
        return 1, 3, 11, hid                             # 33 tokens
    if case == "block_and_one":
        return 1, 1, block + 1, hid
    if case == "padded":
        return 1, 3, 11, hid_from
    cus = torch.cuda.get_device_properties(dev()).multi_processor_count
    n = 1
    while n * 56 * 57 <= block * cus or (n * 56 * 57) % 32 == 0:      # one persistent workgroup a compute unit: more blocks than workgroups, the last one ragged
        n += 1
    return n, 56, 57, hid


@functools.lru_cache(maxsize=None)
def _operands(kernel, case):
    """The case's operands, pack and plain result: made once, shared by the tests, never modified."""
    from recnext_amd import ops
    c = KERNELS[kernel][0]
    n, h, w, hid = _plane(kernel, case)
    z, x, w1, b1, w2, b2 = operands(n, c, hid, h, w, seed=c * 1000 + hid + 7 * h + w)
    hp = ops.channel_mlp_hidden(n * h * w, c, hid, torch.bfloat16)
    assert hp == KERNELS[kernel][1]                      # the padded case runs the same kernel on zero units
    wfrag, bias, hp2 = ops.pack_channel_mlp(w1, b1, w2, b2, hidden_to=hp)
    assert hp2 == hp
    return z, x, w1, b1, w2, b2, wfrag, bias, hp


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_ring_step_against_float64(kernel, case):
    from recnext_amd import ops
    z, x, w1, b1, w2, b2, wfrag, bias, hp = _operands(kernel, case)
    y = ops.channel_mlp(z, x, wfrag, bias, hp)
    assert y.shape == x.shape and y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    check(y, reference(z, x, w1, b1, w2, b2), f"{kernel} {case} {tuple(z.shape)}")


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_ring_step_aliased_call(kernel):
    """z is x: the same tensor is the mixer's input and the residual"""
    from recnext_amd import ops
    z, _, w1, b1, w2, b2, wfrag, bias, hp = _operands(kernel, "block_and_one")
    y = ops.channel_mlp(z, z, wfrag, bias, hp)
    check(y, reference(z, z, w1, b1, w2, b2), f"{kernel} aliased {tuple(z.shape)}")


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_ring_step_repeated_launches_give_equal_bits(kernel):
    """40 launches, equal bits every time: a fragment used before it has arrived, or a ring slot rewritten too early, shows here"""
    from recnext_amd import ops
    z, x, _, _, _, _, wfrag, bias, hp = _operands(kernel, "block_and_one")
    y = ops.channel_mlp(z, x, wfrag, bias, hp)
    outs = [ops.channel_mlp(z, x, wfrag, bias, hp) for _ in range(40)]
    same = torch.stack([(o == y).all() for o in outs]).cpu().tolist()      # one read-back
    assert all(same), f"launches that differ: {[i for i, s in enumerate(same) if not s]}"
