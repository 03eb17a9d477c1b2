"""The fragment packs of the (384, 768) and (512, 768) channel mixers: their size as the library states it and pack_channel_mlp's layout read back on the CPU."""
import pytest
import torch

SHAPES = [(384, 768, 24, 24, 12), (512, 768, 32, 24, 16)]          # C, H, KS1, HT, CT (rcx_mlp.hip mlp_shape)


def test_pack_bytes_of_the_768_wide_mixers():
    from recnext_amd import _lib
    lib = _lib.load()
    assert lib.rcx_channel_mlp_pack_bytes(384, 768) == (24 * 24 + 12 * 2 * 24) * 1024
    assert lib.rcx_channel_mlp_pack_bytes(512, 768) == (24 * 32 + 16 * 2 * 24) * 1024


@pytest.mark.parametrize("c,hp,ks1,ht,ct", SHAPES)
@pytest.mark.parametrize("hidden", [768, 750])
def test_pack_channel_mlp_round_trips(c, hp, ks1, ht, ct, hidden):
    from recnext_amd import ops
    g = torch.Generator().manual_seed(c + hidden)
    w1, b1 = torch.randn(hidden, c, generator=g).bfloat16(), torch.randn(hidden, generator=g).bfloat16()
    w2, b2 = torch.randn(c, hidden, generator=g).bfloat16(), torch.randn(c, generator=g).bfloat16()
    wfrag, bias, got = ops.pack_channel_mlp(w1, b1, w2, b2, hidden_to=hp)
    assert got == hp and wfrag.dtype == torch.bfloat16 and wfrag.numel() * 2 == (ht * ks1 + ct * 2 * ht) * 1024 and bias.numel() == 32 * (ht + ct)
    chunks = wfrag.view(ht, (ks1 + 2 * ct) * 512)
    # W1 fragment (ht, ks), lane (h, m), element j = W1[32 ht + m][16 ks + 8 h + j]
    f1 = chunks[:, :ks1 * 512].reshape(ht, ks1, 2, 32, 8)
    w1_back = f1.permute(0, 3, 1, 2, 4).reshape(32 * ht, 16 * ks1)
    assert torch.equal(w1_back[:hidden, :c], w1) and not bool(w1_back[hidden:].any())
    # W2 fragment (ht, ct, q), lane (h, m), element j = 0.5 W2[32 ct + m][32 ht + unit(8 q + j, h)]
    f2 = chunks[:, ks1 * 512:].reshape(ht, ct, 2, 2, 32, 8)
    w2_back = torch.zeros(32 * ct, 32 * ht)
    for q in range(2):
        for h in range(2):
            for j in range(8):
                w2_back.view(ct, 32, ht, 32)[:, :, :, ops._mlp_acc_unit(8 * q + j, h)] = f2[:, :, q, h, :, j].permute(1, 2, 0).float()
    assert torch.equal(2.0 * w2_back[:c, :hidden], w2.float()) and not bool(w2_back[:, hidden:].any())
    assert torch.equal(bias[:hidden], b1.float()) and not bool(bias[hidden:hp].any()) and torch.equal(bias[hp:hp + c], b2.float())


def test_tile_rule_is_the_librarys():
    """ops._mlp_tiles (Python) and mlp_shape (rcx_mlp.hip) state the same (KS1, HT, CT) rule: the pack they imply has the size the library reports."""
    from recnext_amd import _lib, ops
    lib = _lib.load()
    for c in range(8, 641, 8):
        for hidden in (32, 96, 256, 768, 1024):
            ks1, ht, ct = ops._mlp_tiles(c, hidden)
            assert (ht * ks1 + 2 * ct * ht) * 1024 == lib.rcx_channel_mlp_pack_bytes(c, hidden), (c, hidden)
