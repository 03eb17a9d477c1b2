"""CPU: the LSNet-style RecNeXt-T / S / B (recnext_amd.lsmodels) against the reference's fixtures (tests/golden/ls_*, make_golden_ls.py): parameter
counts, state_dict keys before and after replace_batchnorm, the tiny model's logits, the operator restatement tests/ls_eager.py, the support
queries of the HIP token half at 224 and 256, and the paths that must raise."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from recnext_amd import _lib, lsmodels, models
from tests.ls_eager import eager_token_mixer, token_half
from tests.util import GOLDEN

NAMES = ("recnext_t", "recnext_s", "recnext_b")
PARAMS = {"recnext_t": (12729296, 12112520), "recnext_s": (16485584, 15847976), "recnext_b": (19927632, 19251752)}


def block_cases():
    return sorted(os.path.basename(p)[len("ls_block_"):-4] for p in glob.glob(os.path.join(GOLDEN, "ls_block_*.npz")))


def load_block(name):
    d = np.load(os.path.join(GOLDEN, f"ls_block_{name}.npz"))
    meta = json.loads(str(d["meta"]))
    x = torch.from_numpy(d["x_bf16"].view(np.int16).copy()).view(torch.bfloat16).float()
    sd = {k[4:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd::")}
    return x, torch.from_numpy(d["r"]), torch.from_numpy(d["t_s"]), sd, meta


def build_block(meta, sd, token_mixer=None):
    """An lsmodels.MetaNeXtBlock with the fixture's rep_mixer / token_mixer parameters (the channel mixer is not part of the token half)."""
    blk = lsmodels.MetaNeXtBlock(meta["C"], meta["mlp_ratio"], num_heads=meta["num_heads"], stage=meta["stage"], token_mixer=token_mixer).eval()
    missing, unexpected = blk.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("channel_mixer.") for k in missing), (missing, unexpected)
    return blk


def close(got, want, rel=1e-5):
    return float((got - want).abs().max()) <= rel * max(1e-30, float(want.abs().max()))


@pytest.mark.parametrize("name", NAMES)
def test_parameter_counts(name):
    net = models.create_model(name)
    assert sum(p.numel() for p in net.parameters()) == PARAMS[name][0]
    models.replace_batchnorm(net.eval())
    assert sum(p.numel() for p in net.parameters()) == PARAMS[name][1]


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_keys_match_the_reference(name):
    with open(os.path.join(GOLDEN, "ls_models.json")) as f:
        ref = json.load(f)[name]
    net = models.create_model(name)
    assert list(net.state_dict().keys()) == ref["keys"]
    assert ref["params"] == PARAMS[name][0] and ref["fused_params"] == PARAMS[name][1]
    models.replace_batchnorm(net.eval())
    assert list(net.state_dict().keys()) == ref["fused_keys"]


@pytest.mark.parametrize("name", NAMES)
def test_eager_override_has_the_same_keys(name):
    a = models.create_model(name).state_dict()
    b = models.create_model(name, token_mixer=eager_token_mixer).state_dict()
    assert list(a.keys()) == list(b.keys()) and all(a[k].shape == b[k].shape for k in a)


def test_distillation_recipe():
    assert models.create_model("recnext_b").stages[3].blocks[-1].drop_path.drop_prob == pytest.approx(0.2)
    assert isinstance(models.create_model("recnext_b", distillation=True).stages[3].blocks[-1].drop_path, torch.nn.Identity)
    assert models.create_model("recnext_s", distillation=True).head.distillation


def _tiny(token_mixer=None):
    return lsmodels.RecNext(embed_dim=(16, 32, 48, 64), depth=(1, 1, 1, 1), mlp_ratios=(2, 2, 2, 1.5), num_heads=(1, 1, 1, 2), split_rates=(4, 4, 4, 4),
                            num_classes=10, token_mixer=token_mixer).eval()


def test_tiny_model_logits_and_replace_batchnorm():
    d = np.load(os.path.join(GOLDEN, "ls_tiny_model.npz"))
    sd = {k[4:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd::")}
    hip = _tiny()
    hip.load_state_dict(sd, strict=True)                    # a reference checkpoint loads into the HIP model as it is
    net = _tiny(eager_token_mixer)
    net.load_state_dict(sd, strict=True)
    x = torch.from_numpy(d["x"])
    with torch.no_grad():
        assert close(net(x), torch.from_numpy(d["logits"]))
        models.replace_batchnorm(net)
        assert close(net(x), torch.from_numpy(d["logits_fused"]))
    assert isinstance(net.stages[0].blocks[0].rep_mixer, torch.nn.Conv2d) and net.stages[0].blocks[0].rep_mixer.bias is not None


@pytest.mark.parametrize("name", block_cases())
def test_eager_token_half_matches_the_reference(name):
    x, r, t_s, sd, meta = load_block(name)
    blk = build_block(meta, sd, eager_token_mixer)
    with torch.no_grad():
        got_r, got_t = token_half(blk, x)
    s = meta["split"]
    assert close(got_r, r) and close(got_t[:, :s], t_s)
    assert torch.equal(got_t[:, s:], got_r[:, s:])


def test_rep_fold_is_the_same_either_way():
    """The pack the HIP entry reads is bit-identical before and after replace_batchnorm (both come from _fold_rep in float32)."""
    _, _, _, sd, meta = load_block("14x14_c256")
    blk = build_block(meta, sd)
    w0, b0 = lsmodels._rep_params(blk.rep_mixer)
    models.replace_batchnorm(blk)
    w1, b1 = lsmodels._rep_params(blk.rep_mixer)
    assert torch.equal(w0, w1) and torch.equal(b0, b1)


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    return _lib.load()


def _supported(lib, shape, batch, dtype=1):
    stage, h, w, c, split, heads, kind, _ = shape
    fn = lib.rcx_ls_la3_supported if kind == "la3" else lib.rcx_ls_recattn_supported
    return fn(batch, h, w, c, split, heads, dtype) == 1


@pytest.mark.parametrize("name", NAMES)
def test_every_mixer_shape_is_supported_at_224(lib, name):
    shapes = lsmodels.mixer_shapes(name, 224)
    assert len(shapes) == (4 if name == "recnext_b" else 3)
    for shape in shapes:
        for batch in (1, 3, 256):
            for dt in (0, 1, 2):
                assert _supported(lib, shape, batch, dt), (shape, batch, dt)


def test_the_table_of_mixer_shapes():
    assert lsmodels.mixer_shapes("recnext_t") == [(1, 14, 14, 128, 32, 1, "recattn", 2), (2, 7, 7, 256, 64, 1, "recattn", 8), (3, 4, 4, 512, 128, 1, "la3", 10)]
    assert lsmodels.mixer_shapes("recnext_s") == [(1, 14, 14, 256, 64, 1, "recattn", 2), (2, 7, 7, 384, 96, 1, "recattn", 8), (3, 4, 4, 512, 128, 1, "la3", 10)]
    assert lsmodels.mixer_shapes("recnext_b") == [(0, 28, 28, 128, 32, 1, "recattn", 2), (1, 14, 14, 256, 64, 1, "recattn", 8),
                                                  (2, 7, 7, 384, 96, 1, "recattn", 8), (3, 4, 4, 512, 128, 1, "la3", 12)]


@pytest.mark.parametrize("name", NAMES)
def test_every_mixer_shape_runs_or_falls_back_at_256(lib, name):
    for shape in lsmodels.mixer_shapes(name, 256):
        _, h, w, c, split, heads, kind, _ = shape
        assert _supported(lib, shape, 256) or (kind == "recattn" and split // heads <= 64), shape
    # B's 32 x 32 stage-0 slice does not fit the LDS: the fallback takes it
    assert not _supported(lib, (0, 32, 32, 128, 32, 1, "recattn", 2), 1)


def test_support_queries_refuse(lib):
    assert lib.rcx_ls_recattn_supported(1, 14, 14, 256, 64, 2, 1) == 0          # one head only
    assert lib.rcx_ls_recattn_supported(1, 14, 14, 254, 62, 1, 1) == 0          # channels in fours
    assert lib.rcx_ls_recattn_supported(1, 14, 14, 256, 64, 1, 7) == 0          # dtype
    assert lib.rcx_ls_la3_supported(1, 9, 9, 512, 128, 1, 1) == 0               # more than 64 tokens
    assert lib.rcx_ls_la3_supported(1, 4, 4, 512, 128, 3, 1) == 0               # split not a multiple of 2 heads


def _hip_block():
    _, _, _, sd, meta = load_block("7x7_c256")
    return build_block(meta, sd), meta


def test_cpu_forward_raises():
    blk, meta = _hip_block()
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU only"):
        blk(torch.randn(1, meta["C"], 7, 7))


def test_training_and_gradient_paths_raise():
    blk, meta = _hip_block()
    x = torch.randn(1, meta["C"], 7, 7)
    with pytest.raises(NotImplementedError, match="training"):
        blk(x)                                              # parameters require grad: the forward needs a gradient
    blk.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="training"):
        blk(x)
    blk.eval().requires_grad_(False)
    with pytest.raises(NotImplementedError, match="training"):
        blk(x.requires_grad_())


def test_existing_names_unchanged():
    assert sorted(models.CONFIGS) == sorted([f"recnext_{f}{i}" for f in "ma" for i in range(6)])
    assert type(models.create_model("recnext_a0")) is models.RecNext
    with pytest.raises(KeyError):
        models.create_model("recnext_x")
