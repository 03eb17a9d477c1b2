"""CPU: the grouped Downsample conv of RecNeXt-T / S / B (rcx_grouped_conv2d_fwd, ops.grouped_conv2d, lsmodels.Downsample after
models.use_hip_downsample): the support query, the argument errors that come before any HIP call, the pack layout, the reroute's bookkeeping
(count, state_dict keys, strict loads in both orders, unchanged CPU logits) and the fold's bit-identity."""
import ctypes
import os

import numpy as np
import pytest
import torch

from recnext_amd import _lib, lsmodels, models, ops
from tests.ls_eager import eager_token_mixer
from tests.ls_share_eager import eager_share_token_mixer
from tests.test_ls_share_cpu import NAMES as SHARE_NAMES
from tests.test_ls_share_cpu import load_tiny as load_share_tiny
from tests.test_ls_share_cpu import tiny as share_tiny
from tests.test_lsnet_cpu import NAMES, _tiny, close
from tests.util import GOLDEN

ALL_NAMES = tuple(NAMES) + tuple(SHARE_NAMES)

# (Cin, Cout, groups) of every Downsample of the six registered models and the plane it sees at 224 x 224
REGISTERED = [(64, 128, 64, 28), (128, 256, 128, 14), (256, 512, 256, 7),          # T: 1 -> 2
              (128, 256, 128, 28), (256, 384, 128, 14), (384, 512, 128, 7)]        # S / B: 1 -> 2, 2 -> 3, 3 -> 4


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    return _lib.load()


def test_symbols_and_abi(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("rcx_grouped_conv2d_supported", "rcx_grouped_conv2d_fwd"):
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
    assert lib.rcx_abi_version() == _lib.ABI_VERSION
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "recnext_amd.h")) as f:
        header = f.read()
    assert "lsnet/model/recattn.py:254-263" in header and "recattn_share_channel.py:223-232" in header


def test_supported_answers_for_the_registered_shapes(lib):
    q = lib.rcx_grouped_conv2d_supported
    for cin, cout, g, side in REGISTERED:
        for dt in (0, 1, 2):
            for n in (1, 256):
                assert q(n, side, side, cin, cout, g, 5, 2, dt) == 1, (cin, cout, g, side, dt, n)
            assert q(1, 37, 50, cin, cout, g, 5, 2, dt) == 1                  # any H x W
            assert q(1, 1, 1, cin, cout, g, 5, 2, dt) == 1
    for ci in (1, 2, 3, 4):
        for co in (1, 2, 3, 4):
            assert q(2, 9, 13, 70 * ci, 70 * co, 70, 5, 2, 1) == 1            # groups need not be a multiple of the wave
    assert q(2, 14, 14, 256, 384, 128, 3, 2, 1) == 0                          # k = 3
    assert q(2, 14, 14, 256, 384, 128, 5, 1, 1) == 0                          # stride 1
    assert q(2, 14, 14, 80, 32, 16, 5, 2, 1) == 0                             # ci = 5
    assert q(2, 14, 14, 32, 80, 16, 5, 2, 1) == 0                             # co = 5
    assert q(2, 14, 14, 250, 384, 128, 5, 2, 1) == 0                          # Cin % groups
    assert q(2, 14, 14, 256, 380, 128, 5, 2, 1) == 0                          # Cout % groups
    assert q(2, 14, 14, 256, 384, 128, 5, 2, 3) == 0                          # dtype
    assert q(0, 14, 14, 256, 384, 128, 5, 2, 1) == 0
    assert ops.grouped_conv2d_supported(2, 14, 14, 256, 384, 128, 5, 2, torch.bfloat16)
    assert not ops.grouped_conv2d_supported(2, 14, 14, 256, 384, 128, 5, 2, torch.float64)


def test_the_answer_does_not_depend_on_the_batch(lib):
    q = lib.rcx_grouped_conv2d_supported
    for cin, cout, g, side in REGISTERED:
        assert len({q(n, side, side, cin, cout, g, 5, 2, 1) for n in (1, 2, 3, 64, 256, 1024)}) == 1


def test_argument_errors_without_a_gpu(lib):
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(4)]                  # distinct, aligned, never dereferenced: the checks come first
    fwd = lib.rcx_grouped_conv2d_fwd
    shape = (2, 14, 14, 256, 384, 128, 5, 2, 1)
    assert fwd(None, *p[1:], *shape, None) == _lib.ERR_BAD_ARG
    assert b"null" in lib.rcx_last_error()
    assert fwd(p[0], None, *p[2:], *shape, None) == _lib.ERR_BAD_ARG
    assert fwd(*p[:2], None, p[3], *shape, None) == _lib.ERR_BAD_ARG
    assert fwd(p[0], p[0], *p[2:], *shape, None) == _lib.ERR_BAD_ARG         # y aliases x
    assert b"alias" in lib.rcx_last_error()
    assert fwd(*p[:2], p[1], p[3], *shape, None) == _lib.ERR_BAD_ARG         # the pack aliases y
    assert fwd(*p[:3], p[1], *shape, None) == _lib.ERR_BAD_ARG               # the bias aliases y
    assert fwd(*p[:4], 2, 14, 14, 256, 384, 128, 5, 2, 9, None) == _lib.ERR_BAD_ARG          # dtype
    assert fwd(*p[:4], 2, 0, 14, 256, 384, 128, 5, 2, 1, None) == _lib.ERR_BAD_ARG
    assert fwd(ctypes.c_void_p(4097), *p[1:], *shape, None) == _lib.ERR_BAD_ARG              # half an element
    assert b"aligned" in lib.rcx_last_error()
    # geometry without a kernel
    assert fwd(*p[:4], 2, 14, 14, 256, 384, 128, 3, 2, 1, None) == _lib.ERR_UNSUPPORTED      # k = 3
    assert fwd(*p[:4], 2, 14, 14, 256, 384, 128, 5, 1, 1, None) == _lib.ERR_UNSUPPORTED      # stride 1
    assert fwd(*p[:4], 2, 14, 14, 80, 32, 16, 5, 2, 1, None) == _lib.ERR_UNSUPPORTED         # ci = 5
    assert fwd(*p[:4], 2, 14, 14, 250, 384, 128, 5, 2, 1, None) == _lib.ERR_UNSUPPORTED      # Cin % groups
    assert b"groups" in lib.rcx_last_error()


def test_pack_grouped_weight_is_the_index_formula():
    g, ci, co, k = 5, 3, 4, 5
    w = torch.randn(g * co, ci, k, k, generator=torch.Generator().manual_seed(0)).bfloat16()
    pack = ops.pack_grouped_weight(w)
    assert pack.dtype == torch.float32 and tuple(pack.shape) == (k, k, ci, g * co) and pack.is_contiguous()
    flat = pack.reshape(-1)
    for o in range(g * co):
        for j in range(ci):
            for ky in range(k):
                for kx in range(k):
                    assert float(flat[((ky * k + kx) * ci + j) * (g * co) + o]) == float(w[o, j, ky, kx])
    with pytest.raises(ValueError):
        ops.pack_grouped_weight(w[0])


def test_grouped_conv2d_refuses_a_cpu_tensor():
    w = ops.pack_grouped_weight(torch.randn(64, 3, 5, 5))
    with pytest.raises(_lib.RcxError):
        ops.grouped_conv2d(torch.randn(1, 48, 7, 7), w, None, 16)
    with pytest.raises(ValueError):
        ops.grouped_conv2d(torch.randn(48, 7, 7), w, None, 16)
    with pytest.raises(ValueError):
        ops.grouped_conv2d(torch.randn(1, 48, 7, 7).double(), w, None, 16)


def _downsamples(net):
    return [m for m in net.modules() if isinstance(m, lsmodels.Downsample)]


@pytest.mark.parametrize("name", ALL_NAMES)
def test_use_hip_downsample_counts_and_keeps_the_keys(name):
    net = models.create_model(name).eval()
    keys = list(net.state_dict().keys())
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    assert models.use_hip_downsample(net) == 3
    assert models.use_hip_downsample(net) == 0
    assert all(m._hip is True for m in _downsamples(net)) and len(_downsamples(net)) == 3
    assert list(net.state_dict().keys()) == keys
    net.load_state_dict(sd, strict=True)                                      # rerouted first, loaded second
    other = models.create_model(name).eval()
    other.load_state_dict(net.state_dict(), strict=True)                      # and a rerouted model's checkpoint into a plain one
    models.use_hip_downsample(other)
    fused_keys = list(models.replace_batchnorm(models.create_model(name).eval()).state_dict().keys())
    models.replace_batchnorm(net)
    assert list(net.state_dict().keys()) == fused_keys
    assert models.use_hip_downsample(net) == 0                                # the flag lives on the Downsample, not on the child that was replaced
    plain = models.replace_batchnorm(models.create_model(name).eval())
    assert models.use_hip_downsample(plain) == 3                              # and a folded model is rerouted as well


def test_a_plain_model_is_not_rerouted():
    net = models.create_model("recnext_t")
    assert all(m._hip is False for m in _downsamples(net))


def test_a_replaced_child_is_left_alone():
    net = _tiny()
    net.stages[1].downsample.token_mixer = torch.nn.Identity()
    assert models.use_hip_downsample(net) == 2


def test_cpu_forward_of_the_tiny_model_is_unchanged():
    """A CPU tensor keeps the library conv: the rerouted tiny model (slice mixers restated on operators, which is what runs on a CPU) still
    reproduces the reference's logits under the bar of tests/test_lsnet_cpu.py."""
    d = np.load(os.path.join(GOLDEN, "ls_tiny_model.npz"))
    sd = {k[4:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd::")}
    net = _tiny(eager_token_mixer)
    net.load_state_dict(sd, strict=True)
    assert models.use_hip_downsample(net) == 3
    x = torch.from_numpy(d["x"])
    with torch.no_grad():
        assert close(net(x), torch.from_numpy(d["logits"]))
        models.replace_batchnorm(net)
        assert close(net(x), torch.from_numpy(d["logits_fused"]))


def test_cpu_forward_of_the_tiny_share_model_is_unchanged():
    x, logits, logits_fused, sd = load_share_tiny()
    net = share_tiny(eager_share_token_mixer)
    net.load_state_dict(sd, strict=True)
    assert models.use_hip_downsample(net) == 3
    with torch.no_grad():
        assert close(net(x), logits)
        models.replace_batchnorm(net)
        assert close(net(x), logits_fused)


@pytest.mark.parametrize("cin,cout", [(48, 64), (256, 384), (64, 128)])
def test_folded_and_unfolded_packs_are_equal(cin, cout):
    torch.manual_seed(cin)
    m = lsmodels.Downsample(cin, cout).eval()
    for bn in (b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)):
        bn.running_mean.normal_(0, 0.1)
        bn.running_var.uniform_(0.5, 1.5)
        bn.weight.data.uniform_(0.5, 1.5)
        bn.bias.data.normal_(0, 0.1)
    w0, b0 = m.packed_params()
    assert m.packed_params()[0] is w0                                         # cached while nothing changes
    ci = cin // m.token_mixer.conv.groups
    assert w0.dtype == torch.float32 and tuple(w0.shape) == (5, 5, ci, cout) and b0.dtype == torch.float32 and tuple(b0.shape) == (cout,)
    models.replace_batchnorm(m)
    assert isinstance(m.token_mixer, torch.nn.Conv2d)
    w1, b1 = m.packed_params()
    assert w1 is not w0 and torch.equal(w0, w1) and torch.equal(b0, b1)
    with torch.no_grad():
        m.token_mixer.weight.mul_(2.0)                                        # an in-place change rebuilds the pack
    w2, _ = m.packed_params()
    assert torch.equal(w2, 2.0 * w1)
