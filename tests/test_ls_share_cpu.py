"""CPU: the share-channel RecNeXt-T / S / B (recnext_amd.lsshare) against the reference's fixtures (tests/golden/ls_share_*, make_golden_ls_share.py):
state_dict keys and parameter counts before and after replace_batchnorm, which blocks are share blocks, the tiny model's logits on the operator
restatement tests/ls_share_eager.py, the block fixtures, mixer_shapes, rcx_ls_share_* without a GPU and the paths of ls_share that must raise."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from recnext_amd import _lib, lsmodels, lsshare, models
from tests.ls_eager import token_half
from tests.ls_share_eager import eager_share_token_mixer, share_stage_forward, share_token_half
from tests.test_lsnet_cpu import close
from tests.util import GOLDEN

NAMES = ("recnext_t_share_channel", "recnext_s_share_channel", "recnext_b_share_channel")
TINY = dict(embed_dim=(32, 64, 96, 128), depth=(1, 1, 2, 6), mlp_ratios=(2, 2, 2, 1.5), split_rates=(4, 4, 4, 4), num_classes=10)


def _bf16(a):
    return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16).float()


def load_share_block(name):
    """(x, [x1] * 4, r, t, state_dict, meta) of a share-block fixture; x and the x1 are bf16-representable."""
    d = np.load(os.path.join(GOLDEN, f"ls_share_block_{name}.npz"))
    meta = json.loads(str(d["meta"]))
    sd = {k[4:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd::")}
    return _bf16(d["x_bf16"]), [_bf16(d[f"x1_{j}_bf16"]) for j in range(4)], torch.from_numpy(d["r"]), torch.from_numpy(d["t"]), sd, meta


def build_share_block(meta, sd, hip=True):
    blk = lsshare.ShareBlock(meta["C"], meta["mlp_ratio"], hip=hip).eval()
    missing, unexpected = blk.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("channel_mixer.") for k in missing), (missing, unexpected)
    return blk


def load_la3_block(name):
    """(x, r, t_s, state_dict, meta) of a stage-2 mixer-block fixture, the ls_block_* format."""
    d = np.load(os.path.join(GOLDEN, f"ls_share_la3_{name}.npz"))
    meta = json.loads(str(d["meta"]))
    sd = {k[4:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd::")}
    return _bf16(d["x_bf16"]), torch.from_numpy(d["r"]), torch.from_numpy(d["t_s"]), sd, meta


def build_la3_block(meta, sd, token_mixer=None):
    blk = lsshare.MetaNeXtBlock(meta["C"], meta["mlp_ratio"], stage=meta["stage"], token_mixer=token_mixer).eval()
    missing, unexpected = blk.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("channel_mixer.") for k in missing), (missing, unexpected)
    return blk


def load_tiny():
    """(x, logits, logits_fused, state_dict) of the tiny model; the parameters lie in two files."""
    d = np.load(os.path.join(GOLDEN, "ls_share_tiny_model.npz"))
    d3 = np.load(os.path.join(GOLDEN, "ls_share_tiny_model_stage3.npz"))
    sd = {k[len("sd_bf16::"):]: _bf16(f[k]) for f in (d, d3) for k in f.files if k.startswith("sd_bf16::")}
    return _bf16(d["x_bf16"]), torch.from_numpy(d["logits"]), torch.from_numpy(d["logits_fused"]), sd


def tiny(token_mixer=None):
    return lsshare.RecNext(token_mixer=token_mixer, **TINY).eval()


def _ref(name):
    with open(os.path.join(GOLDEN, "ls_share_models.json")) as f:
        return json.load(f)[name]


@pytest.mark.parametrize("name", NAMES)
def test_keys_and_parameter_counts_match_the_reference(name):
    ref = _ref(name)
    net = models.create_model(name)
    assert type(net) is lsshare.RecNext
    assert list(net.state_dict().keys()) == ref["keys"]
    assert sum(p.numel() for p in net.parameters()) == ref["params"]
    models.replace_batchnorm(net.eval())
    assert list(net.state_dict().keys()) == ref["fused_keys"]
    assert sum(p.numel() for p in net.parameters()) == ref["fused_params"]
    eager = models.create_model(name, token_mixer=eager_share_token_mixer).state_dict()
    assert list(eager.keys()) == ref["keys"]


@pytest.mark.parametrize("name", NAMES)
def test_block_kinds(name):
    net = models.create_model(name)
    depth = lsshare.SHARE_CONFIGS[name]["depth"]
    assert depth[3] == (12 if name == "recnext_b_share_channel" else 10)
    for i, stage in enumerate(net.stages):
        share = [j for j, b in enumerate(stage.blocks) if b.is_share_block]
        assert share == ([4, 9] if i == 3 else []), (i, share)
        for b in stage.blocks:
            assert isinstance(b, lsmodels.MetaNeXtBlock)                        # models._mlp_hosts() sees every block
            if b.is_share_block:
                assert isinstance(b.token_mixer, lsshare.ShareChannelOperation) and not list(b.token_mixer.parameters())
                assert {k.split(".")[0] for k in b.state_dict()} == {"rep_mixer", "channel_mixer"}
            elif i >= 2:
                attn = b.token_mixer.attn
                assert type(attn) is lsmodels.LinearAttention3 and attn.num_heads == 1
                s = b.token_mixer.split_idx
                assert attn.head_dim == s // 2 and attn.qk.conv.weight.shape == (s, s, 1, 1)
            else:
                assert type(b.token_mixer.attn) is lsmodels.LsRecAttn2d and b.token_mixer.attn.down[1].num_heads == 1


def test_recipe_and_names():
    assert models.create_model("recnext_b_share_channel").stages[3].blocks[-1].drop_path.drop_prob == pytest.approx(0.2)
    assert models.create_model("recnext_s_share_channel").stages[3].blocks[-1].drop_path.drop_prob == pytest.approx(0.1)
    assert isinstance(models.create_model("recnext_b_share_channel", distillation=True).stages[3].blocks[-1].drop_path, torch.nn.Identity)
    assert models.create_model("recnext_s_share_channel", distillation=True).head.distillation
    assert models.create_model("recnext_t_share_channel", num_classes=7).head.head.linear.out_features == 7
    assert type(models.create_model("recnext_t")) is lsmodels.RecNext             # the existing names keep their builders
    with pytest.raises(KeyError):
        models.create_model("recnext_x_share_channel")


def test_tiny_model_loads_and_the_restatement_reproduces_its_logits():
    x, logits, logits_fused, sd = load_tiny()
    hip = tiny()
    hip.load_state_dict(sd, strict=True)                    # a reference checkpoint loads into the HIP model as it is
    assert [b.is_share_block for b in hip.stages[3].blocks] == [False] * 4 + [True, False]
    net = tiny(eager_share_token_mixer)
    net.load_state_dict(sd, strict=True)
    with torch.no_grad():
        assert close(net(x), logits)
        y = net.stem(x)                                     # the same through the restatement's own stage loop
        for stage in net.stages:
            y = share_stage_forward(stage, y)
        assert close(net.forward_head(y), logits)
        models.replace_batchnorm(net)
        assert close(net(x), logits_fused)
    assert isinstance(net.stages[3].blocks[4].rep_mixer, torch.nn.Conv2d)


@pytest.mark.parametrize("name", ["4x4_c512", "3x5_c16"])
def test_eager_share_block_matches_the_reference(name):
    x, x1s, r, t, sd, meta = load_share_block(name)
    assert tuple(x.shape) == (meta["B"], meta["C"], meta["H"], meta["W"]) and all(s.shape[1] == meta["split"] for s in x1s)
    blk = build_share_block(meta, sd, hip=False)
    with torch.no_grad():
        got_r, got_t = share_token_half(blk, x, x1s)
        assert close(got_r, r) and close(got_t, t)
        w0, b0 = lsmodels._rep_params(blk.rep_mixer)
        models.replace_batchnorm(blk)
        w1, b1 = lsmodels._rep_params(blk.rep_mixer)
    assert torch.equal(w0, w1) and torch.equal(b0, b1)      # the pack the HIP entry reads is the same before and after folding


@pytest.mark.parametrize("name", ["14x14_c256", "14x14_c384"])
def test_eager_stage2_token_half_matches_the_reference(name):
    x, r, t_s, sd, meta = load_la3_block(name)
    blk = build_la3_block(meta, sd, eager_share_token_mixer)
    with torch.no_grad():
        got_r, got_t = token_half(blk, x)
    s = meta["split"]
    assert s == meta["C"] // 4 and close(got_r, r) and close(got_t[:, :s], t_s)


def test_mixer_shapes():
    t = lsshare.mixer_shapes("recnext_t_share_channel")
    assert t == [(1, 14, 14, 128, 32, 1, "recattn", 2), (2, 7, 7, 256, 64, 1, "la3", 8), (3, 4, 4, 512, 128, 1, "la3", 8), (3, 4, 4, 512, 128, 0, "share", 2)]
    assert lsshare.mixer_shapes("recnext_s_share_channel", 224) == [(1, 14, 14, 256, 64, 1, "recattn", 2), (2, 7, 7, 384, 96, 1, "la3", 8),
                                                                    (3, 4, 4, 512, 128, 1, "la3", 8), (3, 4, 4, 512, 128, 0, "share", 2)]
    assert lsshare.mixer_shapes("recnext_b_share_channel", (224, 224)) == [(0, 28, 28, 128, 32, 1, "recattn", 2), (1, 14, 14, 256, 64, 1, "recattn", 8),
                                                                           (2, 7, 7, 384, 96, 1, "la3", 8), (3, 4, 4, 512, 128, 1, "la3", 10),
                                                                           (3, 4, 4, 512, 128, 0, "share", 2)]
    assert lsshare.mixer_shapes("recnext_b_share_channel", (320, 480)) == [(0, 40, 60, 128, 32, 1, "recattn", 2), (1, 20, 30, 256, 64, 1, "recattn", 8),
                                                                           (2, 10, 15, 384, 96, 1, "la3", 8), (3, 5, 8, 512, 128, 1, "la3", 10),
                                                                           (3, 5, 8, 512, 128, 0, "share", 2)]
    for name in NAMES:                                       # blocks add up to the depths
        assert sum(s[-1] for s in lsshare.mixer_shapes(name)) == sum(lsshare.SHARE_CONFIGS[name]["depth"])
    with pytest.raises(ValueError):
        lsshare.mixer_shapes("recnext_t_share_channel", (1, 2, 3))
    assert lsmodels.mixer_shapes("recnext_t")[-1] == (3, 4, 4, 512, 128, 1, "la3", 10)       # the other family's table is its own


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    return _lib.load()


def test_symbols_and_abi(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("rcx_ls_share_supported", "rcx_ls_share_fwd"):
        assert hasattr(raw, s) and s in _lib.SIGNATURES, s
    assert lib.rcx_abi_version() == 7 == _lib.ABI_VERSION


def test_every_stage_has_a_kernel(lib):
    for name in NAMES:
        for res in (224, 256, (320, 480), (33, 65)):
            for (_, h, w, c, split, heads, kind, _) in lsshare.mixer_shapes(name, res):
                for batch in (1, 3, 256):
                    for dt in (0, 1, 2):
                        if kind == "share":
                            assert lib.rcx_ls_share_supported(batch, h, w, c, split, 4, dt) == 1
                        elif kind == "la3":
                            assert lib.rcx_ls_la3_tiled_supported(batch, h, w, c, split, heads, dt) == 1
                        else:
                            assert lib.rcx_ls_recattn_tiled_supported(batch, h, w, c, split, heads, dt) == 1
    # the 14 x 14 planes of stage 2 are beyond the one-workgroup entry and stay there
    assert lib.rcx_ls_la3_supported(1, 14, 14, 256, 64, 1, 1) == 0 and lib.rcx_ls_la3_tiled_supported(1, 14, 14, 256, 64, 1, 1) == 1
    assert lib.rcx_ls_la3_supported(1, 14, 14, 384, 96, 1, 1) == 0 and lib.rcx_ls_la3_tiled_supported(1, 14, 14, 384, 96, 1, 1) == 1
    # training: the wide core takes the stage-2 head widths
    assert lib.rcx_linear_attention_wide_supported(2, 196, 32, 64, 1, 0) == 1 and lib.rcx_linear_attention_wide_supported(2, 196, 48, 96, 1, 1) == 1


def test_support_query(lib):
    q = lib.rcx_ls_share_supported
    for dt in (0, 1, 2):
        assert q(256, 4, 4, 512, 128, 4, dt) == 1
        assert q(1, 1, 1, 16, 4, 4, dt) == 1
        assert q(2, 3, 5, 16, 4, 4, dt) == 1
        assert q(1, 14, 9, 24, 12, 2, dt) == 1
        assert q(1, 300, 1, 64, 8, 8, dt) == 1
        assert q(1, 7, 7, 512, 512, 1, dt) == 1
    assert q(1, 4, 4, 24, 6, 4, 1) == 0                      # split 6: not in fours
    assert q(1, 4, 4, 18, 6, 3, 1) == 0                      # neither is C
    assert q(1, 4, 4, 512, 128, 3, 1) == 0                   # 3 x 128 != 512: the wrong total
    assert q(1, 4, 4, 512, 64, 4, 1) == 0
    assert q(1, 4, 4, 36, 4, 9, 1) == 0                      # more than 8 sources
    assert q(1, 4, 4, 16, 4, 0, 1) == 0
    assert q(0, 4, 4, 512, 128, 4, 1) == 0
    assert q(1, 4, 4, 512, 128, 4, 3) == 0 and q(1, 4, 4, 512, 128, 4, -1) == 0      # dtype
    assert q(1 << 14, 16, 16, 512, 128, 4, 1) == 0           # 2^31 elements
    assert q((1 << 14) - 1, 16, 16, 512, 128, 4, 1) == 1


def test_argument_errors_without_a_gpu(lib):
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(12)]                 # distinct, aligned, never dereferenced: the checks come first
    fwd = lib.rcx_ls_share_fwd
    srcs = (ctypes.c_void_p * 4)(*[v.value for v in p[5:9]])
    shape = (2, 4, 4, 512, 128, 1)                                            # B H W C split dtype
    assert fwd(None, *p[1:5], srcs, 4, 512, *shape, None) == _lib.ERR_BAD_ARG
    assert b"null" in lib.rcx_last_error()
    for i in range(1, 5):
        args = list(p[:5])
        args[i] = None
        assert fwd(*args, srcs, 4, 512, *shape, None) == _lib.ERR_BAD_ARG
    assert fwd(*p[:5], None, 4, 512, *shape, None) == _lib.ERR_BAD_ARG
    hole = (ctypes.c_void_p * 4)(p[5].value, None, p[7].value, p[8].value)
    assert fwd(*p[:5], hole, 4, 512, *shape, None) == _lib.ERR_BAD_ARG       # a NULL source
    assert fwd(p[0], p[0], *p[2:5], srcs, 4, 512, *shape, None) == _lib.ERR_BAD_ARG             # r aliases x
    assert fwd(p[0], p[1], p[1], *p[3:5], srcs, 4, 512, *shape, None) == _lib.ERR_BAD_ARG       # t aliases r
    alias = (ctypes.c_void_p * 4)(p[5].value, p[2].value, p[7].value, p[8].value)
    assert fwd(*p[:5], alias, 4, 512, *shape, None) == _lib.ERR_BAD_ARG      # t aliases a source
    # alignment: four elements of the dtype (16 bytes in float32, 8 in the 16-bit types), the packs 16 bytes
    assert fwd(ctypes.c_void_p(4096 + 4), *p[1:5], srcs, 4, 512, *shape, None) == _lib.ERR_BAD_ARG
    assert b"aligned" in lib.rcx_last_error()
    odd = (ctypes.c_void_p * 4)(p[5].value, p[6].value + 2, p[7].value, p[8].value)
    assert fwd(*p[:5], odd, 4, 512, *shape, None) == _lib.ERR_BAD_ARG
    half = (ctypes.c_void_p * 4)(p[5].value, p[6].value + 8, p[7].value, p[8].value)
    assert fwd(*p[:5], half, 4, 512, 2, 4, 4, 512, 128, 0, None) == _lib.ERR_BAD_ARG             # 8 bytes: two float32 elements
    assert fwd(*p[:3], ctypes.c_void_p(4096 * 4 + 8), p[4], srcs, 4, 512, *shape, None) == _lib.ERR_BAD_ARG
    assert fwd(*p[:5], srcs, 4, 512, 2, 4, 4, 512, 128, 9, None) == _lib.ERR_BAD_ARG             # dtype
    assert fwd(*p[:5], srcs, 4, 512, 2, 0, 4, 512, 128, 1, None) == _lib.ERR_BAD_ARG
    # shapes without a kernel
    s6 = (ctypes.c_void_p * 4)(*[v.value for v in p[5:9]])
    assert fwd(*p[:5], s6, 4, 24, 2, 4, 4, 24, 6, 1, None) == _lib.ERR_UNSUPPORTED               # split 6
    assert fwd(*p[:5], srcs, 3, 512, *shape, None) == _lib.ERR_UNSUPPORTED                       # the wrong total
    assert fwd(*p[:5], srcs, 4, 64, *shape, None) == _lib.ERR_UNSUPPORTED                        # stride below split
    assert fwd(*p[:5], srcs, 4, 130, *shape, None) == _lib.ERR_UNSUPPORTED                       # stride not in fours
    assert b"stride" in lib.rcx_last_error()


def _pack(c):
    return torch.zeros(9 * c), torch.zeros(c)


def _cl(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).contiguous(memory_format=torch.channels_last)


def test_cpu_tensors_raise():
    x = _cl(2, 16, 3, 5)
    srcs = [_cl(2, 16, 3, 5)[:, :4] for _ in range(4)]
    with pytest.raises(_lib.RcxError, match="no CPU fallback"):
        lsshare.ls_share(x, *_pack(16), srcs)
    blk = lsshare.ShareBlock(16, 1.5).eval().requires_grad_(False)
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU only"):
        blk(x, srcs)
    with torch.no_grad(), pytest.raises(ValueError, match="x1s is empty"):
        blk(x, [])
    blk.train()
    with pytest.raises(NotImplementedError, match="training"):
        blk(x, srcs)
    net = tiny().requires_grad_(False)
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU only"):
        net(torch.zeros(1, 3, 64, 64))


def test_layouts_the_kernel_cannot_address_raise_before_any_launch():
    """Every case is a ValueError from the checks in front of the GPU test and of every allocation: they raise for CPU tensors too."""
    x = _cl(2, 16, 3, 5)
    w, b = _pack(16)
    good = [_cl(2, 16, 3, 5)[:, :4] for _ in range(4)]
    share = lsshare.ls_share

    def bad(srcs, match, xx=x, ww=w, bb=b):
        with pytest.raises(ValueError, match=match):
            share(xx, ww, bb, srcs)

    bad(good, "4-D", xx=x[0])
    bad(good, "float32, bfloat16 or float16", xx=x.double())
    bad(good, "w_rep", ww=w[:-1])
    bad(good, "b_rep", bb=b.double())
    bad(good, "w_rep", ww=torch.zeros(16, 18)[:, :9])                              # not contiguous
    bad([], "1 .. 8")
    bad(good[0], "list")
    bad(good[:3] + [good[3][0]], "4-D")
    bad(good[:3] + [good[3].bfloat16()], "source 3")                               # another dtype
    bad(good[:3] + [_cl(1, 16, 3, 5)[:, :4]], "batch and plane")
    bad(good[:3] + [_cl(2, 16, 5, 3)[:, :4]], "batch and plane")
    bad(good[:3] + [_cl(2, 16, 3, 5)[:, :8]], "channels")                          # unequal channel counts
    bad(good[:3], "do not fill")                                                   # 3 x 4 != 16
    bad([_cl(2, 24, 3, 5)[:, :6] for _ in range(4)], "multiple of 4", xx=_cl(2, 24, 3, 5), ww=torch.zeros(9 * 24), bb=torch.zeros(24))
    bad(good[:3] + [torch.zeros(2, 4, 3, 5)], "side by side")                      # NCHW: channel stride 15
    bad(good[:3] + [_cl(2, 16, 3, 5)[:, ::4]], "side by side")                     # every fourth channel
    bad(good[:3] + [_cl(2, 16, 3, 7)[:, :4, :, :5]], "pixel-major")                # a crop: rows 7 pixels apart
    bad(good[:3] + [_cl(2, 16, 6, 5)[:, :4, ::2]], "pixel-major")                  # every other row
    bad(good[:3] + [_cl(4, 16, 3, 5)[::2, :4]], "pixel-major")                     # every other image
    bad(good[:3] + [_cl(2, 4, 3, 5)], "one stride")                                # dense among slices
    bad([_cl(2, 6, 3, 5)[:, :4] for _ in range(4)], "multiple of 4")               # pixels 6 elements apart
    # what it does take gets as far as the GPU test
    for srcs in (good, [_cl(2, 4, 3, 5) for _ in range(4)], [_cl(2, 8, 3, 5)[:, :4] for _ in range(4)]):
        with pytest.raises(_lib.RcxError, match="no CPU fallback"):
            share(x, w, b, srcs)
    one = [_cl(1, 16, 1, 1)[:, :4] for _ in range(4)]                              # a single pixel: no stride to read, any is right
    with pytest.raises(_lib.RcxError, match="no CPU fallback"):
        share(_cl(1, 16, 1, 1), w, b, one)
