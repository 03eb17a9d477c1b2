"""CPU: the support queries of RecAttn2d's matrix-core attention for heads of 36 .. 64 channels (RecNeXt-A5: 40 per head on every stage).
The queries are host code of the library; they answer for the shapes the wide-head kernels take and refuse where an LDS or head-size rule does."""
import os

import pytest

from recnext_amd import _lib

BF16, F16, F32 = 1, 2, 0
NEAREST = 1


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    return _lib.load()


# (coarse plane h, w, C, heads, launches): A5's stages 0 / 1 take the two-launch form, stage 2 one launch
@pytest.mark.parametrize("h,w,c,heads,launches", [(28, 28, 80, 2, 2), (14, 14, 160, 4, 2), (7, 7, 320, 8, 1),
                                                   (7, 7, 96, 2, 1), (4, 4, 512, 8, 1), (5, 9, 80, 2, 1), (9, 11, 80, 2, 2), (1, 130, 80, 2, 2),
                                                   (7, 7, 384, 8, 1), (28, 28, 128, 2, 2), (56, 56, 72, 2, 2)],
                         ids=lambda v: str(v))
def test_wide_heads_launches(lib, h, w, c, heads, launches):
    assert lib.rcx_recattn_qkcore_launches(256, h, w, c, heads) == launches
    ws = lib.rcx_recattn_qkcore_workspace_bytes(256, h, w, c, heads)
    assert (ws > 0) == (launches == 2)


def test_wide_heads_workspace_grows_with_the_batch(lib):
    a, b = lib.rcx_recattn_qkcore_workspace_bytes(1, 28, 28, 80, 2), lib.rcx_recattn_qkcore_workspace_bytes(256, 28, 28, 80, 2)
    assert a > 0 and b == 256 * a
    # a wide head's partial record is larger than a 32-wide head's on the same plane
    assert a > lib.rcx_recattn_qkcore_workspace_bytes(1, 28, 28, 64, 2)


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_wide_heads_down_qkcore(lib, dt):
    assert lib.rcx_recattn_down_qkcore_supported(256, 14, 14, 320, 8, dt) == 1          # A5 stage 2: one launch from x
    assert lib.rcx_recattn_down_qkcore_supported(256, 14, 14, 160, 4, dt) == 1
    assert lib.rcx_recattn_down_qkcore_supported(256, 7, 7, 320, 8, dt) == 1
    assert lib.rcx_recattn_down_qkcore_supported(256, 14, 14, 320, 8, F32) == 0         # float32 x keeps the float32 chain
    # 8 heads of 64 on the 7 x 7 coarse plane: the true-width float32 image (191 760 B) exceeds the LDS; the plane takes the two-launch form from d
    assert lib.rcx_recattn_down_qkcore_supported(256, 14, 14, 512, 8, dt) == 0
    assert lib.rcx_recattn_qkcore_launches(256, 7, 7, 512, 8) == 2
    assert lib.rcx_recattn_down_qkcore_supported(256, 28, 28, 160, 4, dt) == 0          # no 28 x 28 form


@pytest.mark.parametrize("h,w", [(7, 7), (14, 14), (28, 28)])
def test_wide_heads_refusals(lib, h, w):
    for c, heads in [(136, 2), (272, 4), (76, 2), (152, 4)]:                             # D = 68 (too wide), D = 38 (not a multiple of 4)
        assert lib.rcx_recattn_qkcore_launches(256, h, w, c, heads) == 0
        assert lib.rcx_recattn_qkcore_workspace_bytes(256, h, w, c, heads) == 0
        assert lib.rcx_recattn_down_qkcore_supported(256, 2 * h, 2 * w, c, heads, BF16) == 0
    assert lib.rcx_recattn_qkcore_launches(256, h, w, 40, 1) == 0                        # one wide head: its halves are not whole heads
    assert lib.rcx_recattn_qkcore_launches(256, h, w, 640, 16) == 0                      # 16 wide heads (A5 stage 3) keep the GEMM path


@pytest.mark.parametrize("hw", [14, 7])
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_whole_unit_keeps_refusing_wide_heads(lib, hw, dt):
    for d in range(36, 65, 4):
        for heads in (2, 4, 8):
            assert lib.rcx_recattn2d_fwd_supported(256, hw, hw, d * heads, heads, NEAREST, dt) == 0
    assert lib.rcx_recattn2d_fwd_supported(256, 14, 14, 256, 8, NEAREST, dt) == 1         # 32-wide heads keep the one-launch unit
