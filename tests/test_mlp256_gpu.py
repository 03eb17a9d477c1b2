"""The 256-channel channel mixer (C = 256, H = 512: the 14 x 14 stage of RecNeXt-M3 / A3, two waves per SIMD, 256 tokens a workgroup) against the float64
formula at the bar of tests/test_mlp_gpu.py: the bench shape (one round), more tokens than one round (the workgroups loop), ragged token counts, fewer tokens
than one workgroup, the hidden layer 480 padded to 512, and repeated launches that must agree bit for bit."""
import pytest
import torch

from tests.mlp_common import check, operands, reference

pytestmark = pytest.mark.gpu


def _run(z, x, w1, b1, w2, b2):
    from recnext_amd import ops
    n, c, h, w = z.shape
    hid = w1.shape[0]
    hp = ops.channel_mlp_hidden(n * h * w, c, hid, torch.bfloat16)
    assert hp == 512
    wfrag, bias, _ = ops.pack_channel_mlp(w1, b1, w2, b2, hidden_to=hp)
    return ops.channel_mlp(z, x, wfrag, bias, hp), (wfrag, bias, hp)


# (n, c, hidden, h, w): M = n h w tokens; one workgroup = 256 tokens, one wave = 32
CASES = [(256, 256, 512, 14, 14),        # the bench shape: 50 176 tokens = 196 workgroups, one round
         (512, 256, 512, 14, 14),        # 392 workgroups: more than one per CU, the workgroups loop over blocks
         (7, 256, 512, 13, 11),          # 1 001 tokens: neither a multiple of 256 nor of 32
         (1, 256, 512, 3, 5),            # 15 tokens: less than one wave's tile
         (2, 256, 480, 14, 14)]          # hidden 480 padded to 512 with zero units


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_channel_mlp_256_against_float64(case):
    n, c, hid, h, w = case
    ops_in = operands(n, c, hid, h, w, seed=c * 1000 + hid + h + n)
    y, _ = _run(*ops_in)
    assert y.shape == ops_in[1].shape and y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    check(y, reference(*ops_in), case)


@pytest.mark.parametrize("case", [(256, 256, 512, 14, 14), (3, 256, 512, 14, 14)], ids=lambda c: "x".join(map(str, c)))
def test_channel_mlp_256_is_deterministic(case):
    n, c, hid, h, w = case
    z, x, w1, b1, w2, b2 = operands(n, c, hid, h, w, seed=5)
    y, (wfrag, bias, hp) = _run(z, x, w1, b1, w2, b2)
    from recnext_amd import ops
    for _ in range(8):
        assert torch.equal(y, ops.channel_mlp(z, x, wfrag, bias, hp)), "not deterministic"
