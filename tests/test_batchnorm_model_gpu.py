"""GPU: whole registered models with every nn.BatchNorm2d rerouted to the HIP BatchNorm (models.use_hip_batchnorm), one training step each at batch 4.

recnext_t in float32 against the unrouted model, each measured from a float64 copy as tests/test_ls_train_gpu.py's whole-model test does: the rerouted
step within 4 x the unrouted step's own distance (the factor that test grants a changed summation order), with that test's floors; loss, every
parameter gradient and the running buffers.  recnext_s under bf16 autocast: finite gradients, cosine >= 0.95 to the unrouted step.  recnext_m3 and a
share-channel model: one float32 step each, to show the router reaches them.  The models are rerouted with all_shapes=True: the routing rule
keeps shapes of batch 64 and more, and these steps run at batch 4."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from recnext_amd import batchnorm, models
from tests.test_ls_train_gpu import _loss, _model_pair

DEV = torch.device("cuda:0")


def _batch(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(4, 3, 224, 224, device=DEV, generator=g)
    return x, x.contiguous(memory_format=torch.channels_last), torch.randint(0, 1000, (4,), device=DEV, generator=g)


def _routed_copy(net):
    routed = copy.deepcopy(net)
    plain = sum(type(m) is nn.BatchNorm2d for m in routed.modules())
    assert plain > 0 and models.use_hip_batchnorm(routed, all_shapes=True) == plain and models.use_hip_batchnorm(routed) == 0
    return routed, plain


def _count_executed(net):
    """Forward hooks on every BatchNorm2d of net: -> the list the hooks append to (one entry a call)."""
    ran = []
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.register_forward_hook(lambda mod, inp, out: ran.append(tuple(inp[0].shape)))
    return ran


def _count_hip_calls(monkeypatch):
    calls = []
    real = batchnorm.BatchNormFn.apply
    monkeypatch.setattr(batchnorm.BatchNormFn, "apply", staticmethod(lambda *a: calls.append(tuple(a[0].shape)) or real(*a)))
    return calls


@pytest.mark.gpu
def test_recnext_t_float32_step_rerouted_against_unrouted(monkeypatch):
    ref, hip = _model_pair("recnext_t")
    ref64 = copy.deepcopy(ref).double()
    routed, plain = _routed_copy(hip)
    x, xcl, y = _batch(5)
    calls, ran = _count_hip_calls(monkeypatch), _count_executed(routed)
    l64, lu = _loss(ref64, x.double(), y), _loss(hip, xcl, y)
    assert not calls                                                           # nothing is rerouted unless asked for
    lr = _loss(routed, xcl, y)
    print(f"  recnext_t: {plain} BatchNorm2d modules, {len(ran)} calls in the step, {len(calls)} on the HIP path")
    assert len(calls) == len(ran) >= plain                                     # every BatchNorm2d call of the step took the HIP path
    for loss in (l64, lu, lr):
        loss.backward()
    dist = lambda a, b: float((a.detach().double() - b.detach().double()).abs().max())
    err = lambda a, b: float((a.detach().double() - b.detach().double()).norm())
    assert dist(lr, l64) <= max(1e-4 * abs(float(l64.detach())), 4 * dist(lu, l64))
    pu, pr = dict(hip.named_parameters()), dict(routed.named_parameters())
    allg = torch.cat([p.grad.flatten() for p in ref64.parameters()])
    rms = float(allg.norm()) / allg.numel() ** 0.5
    for k, p in ref64.named_parameters():
        assert pr[k].grad is not None and pr[k].grad.dtype == pr[k].dtype, k
        bar = max(5e-2 * float(p.grad.norm()), 4 * err(pu[k].grad, p.grad), 1e-2 * rms * p.numel() ** 0.5)
        assert err(pr[k].grad, p.grad) <= bar, (k, err(pr[k].grad, p.grad), err(pu[k].grad, p.grad), float(p.grad.norm()))
    cat = lambda ps: torch.cat([ps[k].grad.flatten() for k, _ in ref64.named_parameters()])
    assert err(cat(pr), allg) <= max(2e-3 * float(allg.norm()), 4 * err(cat(pu), allg))
    bu, br = dict(hip.named_buffers()), dict(routed.named_buffers())
    for k, b in ref64.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(br[k]) == int(bu[k]) == int(b) == 1, k
        elif k.endswith(("running_mean", "running_var")):
            assert err(br[k], b) <= max(1e-4 * float(b.norm()), 4 * err(bu[k], b)), (k, err(br[k], b), err(bu[k], b))


@pytest.mark.gpu
def test_recnext_s_bf16_autocast_step(monkeypatch):
    _, hip = _model_pair("recnext_s")
    routed, plain = _routed_copy(hip)
    _, xcl, y = _batch(6)
    calls, ran = _count_hip_calls(monkeypatch), _count_executed(routed)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lu, lr = _loss(hip, xcl, y), _loss(routed, xcl, y)
    print(f"  recnext_s: {plain} BatchNorm2d modules, {len(ran)} calls in the step, {len(calls)} on the HIP path")
    assert len(calls) == len(ran) >= plain
    lu.backward(), lr.backward()
    assert abs(float(lr) - float(lu)) < 5e-2 * max(1.0, abs(float(lu)))
    pr = dict(routed.named_parameters())
    for k, p in hip.named_parameters():
        assert pr[k].grad is not None and bool(torch.isfinite(pr[k].grad).all()), k
    gu = torch.cat([p.grad.flatten() for p in hip.parameters()])
    gr = torch.cat([pr[k].grad.flatten() for k, _ in hip.named_parameters()])
    assert float(F.cosine_similarity(gu.double(), gr.double(), dim=0)) >= 0.95


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["recnext_m3", "recnext_t_share_channel"])
def test_the_router_reaches_the_other_model_modules(name, monkeypatch):
    torch.manual_seed(0)
    net = models.create_model(name, **({"drop_path": 0.0} if name == "recnext_m3" else {"drop_path_rate": 0.0}))
    net = net.to(DEV).to(memory_format=torch.channels_last).train()
    routed, plain = _routed_copy(net)
    _, xcl, y = _batch(7)
    calls, ran = _count_hip_calls(monkeypatch), _count_executed(routed)
    lu, lr = _loss(net, xcl, y), _loss(routed, xcl, y)
    print(f"  {name}: {plain} BatchNorm2d modules, {len(ran)} calls in the step, {len(calls)} on the HIP path")
    assert len(calls) == len(ran) >= plain
    lu.backward(), lr.backward()
    assert abs(float(lr) - float(lu)) <= 1e-3 * max(1.0, abs(float(lu)))
    pr = dict(routed.named_parameters())
    for k, p in net.named_parameters():
        assert (pr[k].grad is None) == (p.grad is None) and (p.grad is None or bool(torch.isfinite(pr[k].grad).all())), k
    live = [k for k, p in net.named_parameters() if p.grad is not None]
    gu = torch.cat([dict(net.named_parameters())[k].grad.flatten() for k in live])
    gr = torch.cat([pr[k].grad.flatten() for k in live])
    assert float(F.cosine_similarity(gu.double(), gr.double(), dim=0)) >= 0.99
    # the running buffers of both float32 steps within 1e-3 in relative L2, the floor tests/test_ls_train_gpu.py grants a whole float32 model's output
    # after a step (a deep layer's statistics carry the summation-order differences of every layer before it)
    for (k, a), (_, b) in zip(net.named_buffers(), routed.named_buffers()):
        if k.endswith(("running_mean", "running_var")):
            assert float((a.double() - b.double()).norm()) <= 1e-3 * float(a.double().norm()) + 1e-6, k
