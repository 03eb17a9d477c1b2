"""CPU: the input-only RecConv2d backward's C entry points (rcx_recconv2d_bwd_input*): declared, exported, their schedule at every cut-over,
their workspace, and their argument errors -- all answered before any HIP call."""
import ctypes
import os
import re

from recnext_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rcx_recconv2d_bwd_input", "rcx_recconv2d_bwd_input_workspace_bytes", "rcx_recconv2d_bwd_input_gy_dtype", "rcx_recconv2d_bwd_input_plan")
BF16, F16, F32 = _lib.DTYPE_BF16, _lib.DTYPE_F16, _lib.DTYPE_F32


def _plan(n, c, h, level, dtype=BF16):
    return _lib.load().rcx_recconv2d_bwd_input_plan(n, c, h, h, level, 5, dtype).decode()


def test_header_declares_and_library_exports_the_input_backward():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "recnext_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.load().rcx_abi_version() == 7                       # additions only: the ABI version stays


def test_input_backward_plan_at_the_cut_overs():
    """Both sides of each cut-over of the full backward's schedule: the same kinds, without its 512-image limit."""
    lib = _lib.load()
    assert _plan(512, 8, 7, 1) == "one(k_recconv_adj_cpl7)"
    assert _plan(513, 8, 7, 1) == "one(k_recconv_adj_cpl7)"                        # no partial rows: no batch limit ...
    assert lib.rcx_recconv2d_bwd_plan(513, 8, 7, 7, 1, 5, BF16) == b"steps"       # ... where the full backward falls back to the steps
    assert _plan(128, 256, 14, 2) == "one(k_recconv_adj_cpl14)"
    assert _plan(130, 256, 14, 2) == "one(k_recconv_adj_cpl14)"
    assert _plan(64, 64, 56, 4) == "tiled(levels=2)+one(k_recconv_adj_cpl14)"
    assert _plan(288, 128, 28, 3) == "tiled(levels=1)+one(k_recconv_adj_cpl14)"
    assert _plan(1, 16, 112, 5) == "steps+one(k_recconv_adj_cpl14)"               # 112 -> 56 -> 28 -> 14
    assert _plan(1, 8, 40, 5) == "steps"
    assert _plan(2, 16, 14, 1) == "steps"                                          # 14 x 14 at level 1: no one-launch kernel
    assert lib.rcx_recconv2d_bwd_input_plan(2, 64, 56, 56, 9, 5, BF16) == b"invalid"
    for dt in (F32, F16):
        assert _plan(64, 64, 56, 4, dt) == "tiled(levels=2)+one(k_recconv_adj_cpl14)"
        assert _plan(600, 512, 7, 1, dt) == "one(k_recconv_adj_cpl7)"


def test_input_backward_plan_under_the_switches(monkeypatch):
    monkeypatch.setenv("RCX_BWD_FUSED", "0")
    assert _plan(128, 256, 14, 2) == "steps"
    assert _plan(513, 8, 7, 1) == "steps"
    assert _plan(64, 64, 56, 4) == "steps"                                        # no 14 x 14 tail, so no tiled levels either
    assert _plan(1, 16, 112, 5) == "steps"
    monkeypatch.delenv("RCX_BWD_FUSED")
    monkeypatch.setenv("RCX_FORCE_GENERIC", "1")
    assert _plan(512, 8, 7, 1) == "generic"
    assert _plan(64, 64, 56, 4) == "generic"
    assert _plan(1, 8, 40, 5) == "generic"


def test_input_backward_gy_dtype():
    lib = _lib.load()
    q = lambda n, c, h, level, dt: lib.rcx_recconv2d_bwd_input_gy_dtype(n, c, h, h, level, 5, dt)
    for dt in (BF16, F16):                                          # the one-launch and tiled schedules read a 16-bit gy as it is
        assert q(513, 8, 7, 1, dt) == dt
        assert q(130, 256, 14, 2, dt) == dt
        assert q(64, 64, 56, 4, dt) == dt
        assert q(288, 128, 28, 3, dt) == dt
        assert q(1, 16, 112, 5, dt) == F32                          # the per-step schedule: float32
        assert q(1, 8, 40, 5, dt) == F32
        assert q(64, 66, 56, 4, dt) == F32                          # C % 4 != 0: refused by the entry anyway
    assert q(64, 64, 56, 4, F32) == F32
    for n, c, h, level in [(512, 8, 7, 1), (128, 256, 14, 2), (64, 64, 56, 4), (288, 128, 28, 3)]:    # the full backward's bf16 gy stays accepted
        if lib.rcx_recconv2d_bwd_gy_dtype(n, c, h, h, level, 5, BF16) == BF16:
            assert q(n, c, h, level, BF16) == BF16


def test_input_backward_workspace():
    lib = _lib.load()
    ws = lambda n, c, h, level: lib.rcx_recconv2d_bwd_input_workspace_bytes(n, c, h, h, level, 5)
    assert ws(513, 8, 7, 1) == 0 and ws(128, 256, 14, 2) == 0 and ws(4096, 512, 7, 1) == 0
    for n, c, h, level in [(512, 8, 7, 1), (64, 64, 56, 4), (288, 128, 28, 3), (1, 16, 112, 5), (1, 8, 40, 5), (2, 16, 14, 1), (3, 8, 9, 0)]:
        full = lib.rcx_recconv2d_bwd_workspace_bytes(n, c, h, h, level, 5)
        assert 0 <= ws(n, c, h, level) <= full, (n, c, h, level)
    assert ws(64, 64, 56, 4) > 0 and ws(64, 64, 56, 4) < lib.rcx_recconv2d_bwd_workspace_bytes(64, 64, 56, 56, 4, 5)
    assert ws(0, 64, 56, 4) == 0 and ws(2, 64, 56, 9) == 0


def test_input_backward_argument_errors_without_gpu():
    """Each bad argument returns its documented code before anything touches a device (the pointers below are never dereferenced)."""
    lib = _lib.load()
    p = ctypes.c_void_p(0x1000)
    q = ctypes.c_void_p(0x2000)

    def call(gy=p, gy_dt=F32, wpack=p, wflip=p, gx=q, ws=None, nbytes=0, n=2, c=8, h=7, level=1, mode=0, dt=F32):
        return lib.rcx_recconv2d_bwd_input(gy, gy_dt, wpack, wflip, gx, ws, nbytes, n, c, h, h, level, 5, mode, dt, None)

    assert call(gy=None) == _lib.ERR_BAD_ARG
    assert call(gx=None) == _lib.ERR_BAD_ARG
    assert call(wpack=None) == _lib.ERR_BAD_ARG
    assert call(wflip=None) == _lib.ERR_BAD_ARG
    assert call(gx=p) == _lib.ERR_BAD_ARG                          # gx aliasing gy
    assert call(n=0) == _lib.ERR_BAD_ARG
    assert call(level=9) == _lib.ERR_BAD_ARG
    assert call(level=-1) == _lib.ERR_BAD_ARG
    assert call(mode=2) == _lib.ERR_BAD_ARG
    assert call(dt=7) == _lib.ERR_BAD_ARG
    assert call(gy_dt=7) == _lib.ERR_BAD_ARG
    assert call(c=6) == _lib.ERR_UNSUPPORTED                        # C % 4 != 0
    assert call(gy_dt=BF16, dt=F32) == _lib.ERR_UNSUPPORTED        # a 16-bit gy for a float32 block
    assert call(gy_dt=F16, dt=BF16) == _lib.ERR_UNSUPPORTED        # ... or of another 16-bit type
    assert call(gy_dt=BF16, dt=BF16, n=1, c=16, h=112, level=5) == _lib.ERR_WORKSPACE     # the steps need a workspace ...
    need = lib.rcx_recconv2d_bwd_input_workspace_bytes(1, 16, 112, 112, 5, 5)
    assert call(gy_dt=BF16, dt=BF16, n=1, c=16, h=112, level=5, ws=q, nbytes=need) == _lib.ERR_UNSUPPORTED   # ... and read float32 gy only
    assert call(n=1, c=16, h=112, level=5, ws=q, nbytes=need - 1) == _lib.ERR_WORKSPACE
    assert b"gy" in lib.rcx_last_error() or b"workspace" in lib.rcx_last_error()
