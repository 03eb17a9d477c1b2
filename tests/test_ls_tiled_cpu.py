"""CPU: the tiled token half of the LSNet-style RecNeXt-T / S / B (rcx_ls_recattn_tiled_* / rcx_ls_la3_tiled_*): symbols and ABI, the support and
workspace queries on planes the one-workgroup entries refuse, argument errors without a GPU, mixer_shapes on (H, W) pairs, and the large-plane
reference fixtures (tests/golden/ls_tiled_block_*, make_golden_ls_tiled.py) against the operator restatement tests/ls_eager.py."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest
import torch

from recnext_amd import _lib, lsmodels
from tests.ls_eager import eager_token_mixer, token_half
from tests.test_lsnet_cpu import NAMES, build_block, close
from tests.util import GOLDEN

SYMBOLS = ("rcx_ls_recattn_tiled_supported", "rcx_ls_recattn_tiled_workspace_bytes", "rcx_ls_recattn_tiled_fwd",
           "rcx_ls_la3_tiled_supported", "rcx_ls_la3_tiled_workspace_bytes", "rcx_ls_la3_tiled_fwd")
# (H, W, C, split, heads) the issue names
LA3_SHAPES = [(12, 12, 512, 128, 1), (13, 21, 512, 128, 1)]
RECATTN_SHAPES = [(32, 32, 128, 32, 1), (16, 16, 384, 96, 1), (100, 168, 128, 32, 1)]


def tiled_cases():
    return sorted(os.path.basename(p)[len("ls_tiled_block_"):-4] for p in glob.glob(os.path.join(GOLDEN, "ls_tiled_block_*.npz")))


def load_tiled_block(name):
    """(x, r[:, :meta['r_channels']], t_s, state_dict, meta) of a large-plane fixture; x is bf16-representable."""
    d = np.load(os.path.join(GOLDEN, f"ls_tiled_block_{name}.npz"))
    meta = json.loads(str(d["meta"]))
    x = torch.from_numpy(d["x_bf16"].view(np.int16).copy()).view(torch.bfloat16).float()
    sd = {k[4:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd::")}
    return x, torch.from_numpy(d["r"]), torch.from_numpy(d["t_s"]), sd, meta


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    return _lib.load()


def test_symbols_and_abi(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
    assert lib.rcx_abi_version() == 7 == _lib.ABI_VERSION


def test_the_fixture_set():
    assert {"12x12_c512", "9x13_c512", "36x36_c128", "16x16_c384", "25x19_c256"} <= set(tiled_cases())
    biggest = max(os.path.getsize(p) for p in glob.glob(os.path.join(GOLDEN, "ls_block_*.npz")))
    for name in tiled_cases():
        assert os.path.getsize(os.path.join(GOLDEN, f"ls_tiled_block_{name}.npz")) <= biggest, name


def test_queries_on_the_large_planes(lib):
    for (h, w, c, s, heads) in LA3_SHAPES:
        for dt in (0, 1, 2):
            assert lib.rcx_ls_la3_tiled_supported(1, h, w, c, s, heads, dt) == 1
            assert lib.rcx_ls_la3_supported(1, h, w, c, s, heads, dt) == 0                 # the one-workgroup query keeps its answer
            assert lib.rcx_ls_la3_tiled_workspace_bytes(1, h, w, c, s, heads, dt) > 0
    for (h, w, c, s, heads) in RECATTN_SHAPES:
        for dt in (0, 1, 2):
            assert lib.rcx_ls_recattn_tiled_supported(1, h, w, c, s, heads, dt) == 1
            assert lib.rcx_ls_recattn_supported(1, h, w, c, s, heads, dt) == 0
            assert lib.rcx_ls_recattn_tiled_workspace_bytes(1, h, w, c, s, heads, dt) > 0


def test_workspace_is_a_function_of_the_shape_alone(lib):
    """Float32 whatever the I/O dtype, slice channels only, linear in the batch (the schedule of an image never depends on the batch)."""
    for fn, shapes in ((lib.rcx_ls_la3_tiled_workspace_bytes, LA3_SHAPES), (lib.rcx_ls_recattn_tiled_workspace_bytes, RECATTN_SHAPES)):
        for (h, w, c, s, heads) in shapes:
            one = fn(1, h, w, c, s, heads, 1)
            assert one == fn(1, h, w, c, s, heads, 0) == fn(1, h, w, c, s, heads, 2)
            assert fn(1, h, w, c, s, heads, 1) == one                                       # asked again: the same
            assert fn(7, h, w, c, s, heads, 1) == 7 * one
            assert one == fn(1, h, w, 2 * c, s, heads, 1)                                   # the passthrough channels take no workspace
            assert one >= 4 * h * w * s
    # LinearAttention3 at 12 x 12, split 128, one head: the fine slice + 5 chunks of 32 tokens x (64 x 128 of k^T v + 64 of sum(k))
    assert lib.rcx_ls_la3_tiled_workspace_bytes(1, 12, 12, 512, 128, 1, 1) == 4 * (144 * 128 + 5 * (64 * 128 + 64))
    # RecAttn2d at 32 x 32, split 32: the fine slice, d and the attention result at 16 x 16, 4 chunks of 64 tokens x (32 x 32 + 32)
    assert lib.rcx_ls_recattn_tiled_workspace_bytes(1, 32, 32, 128, 32, 1, 1) == 4 * (1024 * 32 + 2 * 256 * 32 + 4 * (32 * 32 + 32))


def test_queries_refuse(lib):
    assert lib.rcx_ls_recattn_tiled_supported(1, 32, 32, 128, 32, 2, 1) == 0         # one head only
    assert lib.rcx_ls_recattn_tiled_supported(1, 32, 32, 126, 30, 1, 1) == 0         # channels in fours
    assert lib.rcx_ls_recattn_tiled_supported(1, 32, 32, 128, 32, 1, 7) == 0         # dtype
    assert lib.rcx_ls_recattn_tiled_supported(0, 32, 32, 128, 32, 1, 1) == 0
    assert lib.rcx_ls_la3_tiled_supported(1, 12, 12, 512, 128, 3, 1) == 0            # split not a multiple of 2 heads
    assert lib.rcx_ls_la3_tiled_supported(1, 12, 12, 512, 128, 2, 1) == 1
    assert lib.rcx_ls_la3_tiled_workspace_bytes(1, 12, 12, 512, 128, 3, 1) == 0
    # tiny and ragged planes have kernels too
    for (h, w) in ((1, 1), (3, 5), (9, 9), (5, 13), (1, 300)):
        assert lib.rcx_ls_la3_tiled_supported(1, h, w, 512, 128, 1, 1) == 1
        assert lib.rcx_ls_recattn_tiled_supported(1, h, w, 256, 64, 1, 1) == 1


def test_argument_errors_without_a_gpu(lib):
    p = [ctypes.c_void_p(16 * (i + 1)) for i in range(16)]                  # distinct, aligned, never dereferenced: the checks come first
    shape = (1, 32, 32, 128, 32, 1, 1)
    need = lib.rcx_ls_recattn_tiled_workspace_bytes(*shape)
    fwd = lib.rcx_ls_recattn_tiled_fwd
    assert fwd(*p[:15], None, 0, *shape, None) == _lib.ERR_WORKSPACE
    assert fwd(*p[:16], need - 4, *shape, None) == _lib.ERR_WORKSPACE
    assert b"workspace" in lib.rcx_last_error()
    assert fwd(None, *p[1:16], need, *shape, None) == _lib.ERR_BAD_ARG
    assert b"null" in lib.rcx_last_error()
    assert fwd(*p[:14], None, p[15], need, *shape, None) == _lib.ERR_BAD_ARG
    assert fwd(p[0], p[0], *p[2:16], need, *shape, None) == _lib.ERR_BAD_ARG                    # r aliases x
    assert fwd(*p[:15], p[2], need, *shape, None) == _lib.ERR_BAD_ARG                           # the workspace aliases t
    assert fwd(ctypes.c_void_p(8), *p[1:16], need, *shape, None) == _lib.ERR_BAD_ARG            # alignment
    assert fwd(*p[:15], ctypes.c_void_p(1000), need, *shape, None) == _lib.ERR_BAD_ARG
    assert fwd(*p[:16], need, 1, 32, 32, 128, 32, 1, 9, None) == _lib.ERR_BAD_ARG               # dtype
    assert fwd(*p[:16], need, 1, 0, 32, 128, 32, 1, 1, None) == _lib.ERR_BAD_ARG
    assert fwd(*p[:16], need, 1, 32, 32, 128, 32, 2, 1, None) == _lib.ERR_UNSUPPORTED           # two heads
    assert fwd(*p[:16], need, 1, 32, 32, 128, 30, 1, 1, None) == _lib.ERR_UNSUPPORTED

    shape3 = (1, 12, 12, 512, 128, 1, 1)
    need3 = lib.rcx_ls_la3_tiled_workspace_bytes(*shape3)
    fwd3 = lib.rcx_ls_la3_tiled_fwd
    assert fwd3(*p[:11], None, 0, *shape3, None) == _lib.ERR_WORKSPACE
    assert fwd3(*p[:12], need3 - 1, *shape3, None) == _lib.ERR_WORKSPACE
    assert fwd3(*p[:5], None, *p[6:12], need3, *shape3, None) == _lib.ERR_BAD_ARG
    assert fwd3(*p[:2], p[1], *p[3:12], need3, *shape3, None) == _lib.ERR_BAD_ARG               # t aliases r
    assert fwd3(*p[:12], need3, 1, 12, 12, 512, 128, 3, 1, None) == _lib.ERR_UNSUPPORTED
    assert fwd3(*p[:12], need3, 1, 12, 12, 512, 128, 1, -1, None) == _lib.ERR_BAD_ARG


@pytest.mark.parametrize("name", NAMES)
def test_every_mixer_shape_has_a_kernel_at_any_size(lib, name):
    for res in (224, 256, 288, 384, 512, (320, 480), (200, 336), (33, 65)):
        for (_, h, w, c, split, heads, kind, _) in lsmodels.mixer_shapes(name, res):
            one, tiled = ((lib.rcx_ls_la3_supported, lib.rcx_ls_la3_tiled_supported) if kind == "la3"
                          else (lib.rcx_ls_recattn_supported, lib.rcx_ls_recattn_tiled_supported))
            for batch in (1, 3, 256):
                assert tiled(batch, h, w, c, split, heads, 1) == 1, (res, h, w, c)
                if res == 224:
                    assert one(batch, h, w, c, split, heads, 1) == 1            # dispatch at 224 stays with the one-workgroup entries


def test_mixer_shapes_takes_a_pair():
    assert lsmodels.mixer_shapes("recnext_t", (224, 224)) == lsmodels.mixer_shapes("recnext_t", 224) == lsmodels.mixer_shapes("recnext_t")
    assert lsmodels.mixer_shapes("recnext_b", (320, 480)) == [(0, 40, 60, 128, 32, 1, "recattn", 2), (1, 20, 30, 256, 64, 1, "recattn", 8),
                                                              (2, 10, 15, 384, 96, 1, "recattn", 8), (3, 5, 8, 512, 128, 1, "la3", 12)]
    assert [s[1:3] for s in lsmodels.mixer_shapes("recnext_t", 384)] == [(24, 24), (12, 12), (6, 6)]
    with pytest.raises(ValueError):
        lsmodels.mixer_shapes("recnext_t", (1, 2, 3))


@pytest.mark.parametrize("name", tiled_cases())
def test_eager_token_half_matches_the_large_plane_fixtures(name):
    x, r, t_s, sd, meta = load_tiled_block(name)
    assert tuple(x.shape) == (1, meta["C"], meta["H"], meta["W"])
    blk = build_block(meta, sd, eager_token_mixer)
    with torch.no_grad():
        got_r, got_t = token_half(blk, x)
    s, rc = meta["split"], meta["r_channels"]
    assert rc >= s + 4 and tuple(r.shape) == (1, rc, meta["H"], meta["W"])
    assert close(got_r[:, :rc], r) and close(got_t[:, :s], t_s)
    assert torch.equal(got_t[:, s:], got_r[:, s:])
