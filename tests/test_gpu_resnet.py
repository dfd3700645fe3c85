"""tadmm/resnet_cifar_layers.py and resnet_inet_layers.py on the device, float32: blocks and whole models with every
BatchNorm tail forced to the launch (csrc/bnact.hip), against the float64 restatement of tests/_resnet_ref.py; the composed
tails are the yardstick under the rule of tests/test_gpu_vit.py, in the max norm: with e_f the launch route's error and
e_c the composed route's, both max |err| / max |float64 value|, e_f <= 2 max(e_c, 2^-23), for the output and every
parameter gradient.  The factorised convolutions are restated too: their dense kernels are the factors multiplied out in
float64 (`_resnet_ref.dense_weight`), and float64 autograd carries the gradients to the factors."""
import pytest
import torch

import _resnet_ref as R
from tadmm import get_hp_dict
from tadmm import resnet_cifar_layers as RC
from tadmm import resnet_inet_layers as RI

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -23


class NoRanks:
    ranks = {}
    tt_shapes = {}


def bar(e_f, e_c, what):
    print(f"    {what:<44s} launch {e_f:.3e}   composed {e_c:.3e}")
    assert e_f <= 2.0 * max(e_c, U), (what, e_f, e_c)
    return e_f


def rel(got, want):
    return float((got.detach().to("cpu", torch.float64) - want.detach()).abs().max()) / float(want.detach().abs().max())


def randomise(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(1 + 0.3 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.bias.shape, generator=g))
    return mod


def both_routes(mod, ref_fn, x, training, what):
    """Output and every parameter gradient of `mod` (on the device) under both routes against `ref_fn(x64, sd, training)`."""
    mod.train(training)
    sd = R.state64(mod, requires_grad=True)
    names = [n for n, _ in mod.named_parameters()]
    want = ref_fn(R.f64(x), sd, training)
    up = torch.randn(want.shape, generator=torch.Generator().manual_seed(1))
    want_g = torch.autograd.grad(want, [sd[n] for n in names], R.f64(up))
    got = {}
    for route in ("launch", "composed"):
        out = mod.set_route(route)(x.to(DEV))
        got[route] = [out] + list(torch.autograd.grad(out, list(mod.parameters()), up.to(DEV)))
    worst = 0.0
    for i, (key, ref) in enumerate(zip(["output"] + names, [want] + list(want_g))):
        worst = max(worst, bar(rel(got["launch"][i], ref), rel(got["composed"][i], ref), f"{what} {key}"))
    print(f"    worst launch error of {what}: {worst:.3e}")


@pytest.mark.parametrize("kind", ["ttm", "dense"])
def test_cifar_block_option_a_against_float64(kind):
    """resnet_cifar_tt.py: TTBasicBlock at stage 2, id 0 (16 -> 32, stride 2, option A) on a (2, 16, 8, 8) input."""
    torch.manual_seed(11)
    hp = get_hp_dict("ttm_resnet32", "3") if kind == "ttm" else NoRanks
    blk = randomise(RC.TTBasicBlock(16, 32, 2, option="A", conv=RC.TTConv2dM, stage=2, id=0, hp_dict=hp), 2).to(DEV)
    assert isinstance(blk.conv1, RC.TTConv2dM) == (kind == "ttm") and isinstance(blk.conv2, RC.TTConv2dM) == (kind == "ttm")
    assert blk.pad == 8
    x = torch.randn(2, 16, 8, 8)
    both_routes(blk, lambda x64, sd, tr: R.cifar_block(x64, sd, "", blk, tr), x, True, f"{kind} option-A block")


def test_inet_bottleneck_with_downsample_against_float64():
    """resnet_inet_tt.py: TTBottleneck at stage 1, id 0 with its downsample, from the ttr_resnet50 general table, on a
    (2, 64, 7, 7) input."""
    torch.manual_seed(12)
    hp = get_hp_dict("ttr_resnet50", "3", tt_type="general")
    ds = torch.nn.Sequential(RI.conv1x1(64, 256, 1), torch.nn.BatchNorm2d(256))
    blk = randomise(RI.TTBottleneck(64, 64, 1, ds, stage=1, id=0, conv=RI.TTConv2dR, hp_dict=hp), 3).to(DEV)
    assert isinstance(blk.conv2, RI.TTConv2dR) and isinstance(blk.conv1, torch.nn.Conv2d)
    x = torch.randn(2, 64, 7, 7)
    both_routes(blk, lambda x64, sd, tr: R.inet_block(x64, sd, "", blk, tr), x, True, "ttr bottleneck")


@pytest.mark.parametrize("case", [("tkc_resnet32", "3", RC, (2, 3, 32, 32)), ("ttm_resnet18", "2", RI, (2, 3, 64, 64))],
                         ids=lambda c: c[0])
def test_whole_model_training_step_and_eval_forward(case):
    name, ratio, mod, shape = case
    torch.manual_seed(13)
    model = randomise(getattr(mod, name)(get_hp_dict(name, ratio), num_classes=10), 4).to(DEV)
    ref_fn = R.cifar_resnet if mod is RC else R.inet_resnet
    img = torch.randn(shape)
    # the eval forward against float64, both routes
    model.eval()
    want = ref_fn(R.f64(img), R.state64(model), model, False)
    with torch.no_grad():
        got = {route: model.set_route(route)(img.to(DEV)) for route in ("launch", "composed")}
    assert got["launch"].shape == (2, 10)
    bar(rel(got["launch"], want), rel(got["composed"], want), f"{name} eval logits")
    # one training step: the logits against float64, every parameter with a finite gradient, the buffers updated
    model.train()
    want = ref_fn(R.f64(img), R.state64(model), model, True)
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "tracked" in k}
    outs = {}
    for route in ("launch", "composed"):
        model.load_state_dict(before, strict=False)
        model.zero_grad(set_to_none=True)
        out = model.set_route(route)(img.to(DEV))
        out.square().mean().backward()
        outs[route] = (out.detach(), {k: v.clone() for k, v in model.state_dict().items() if k in before},
                       {n: p.grad.clone() for n, p in model.named_parameters()})
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    bar(rel(outs["launch"][0], want), rel(outs["composed"][0], want), f"{name} training logits")
    for k, v in outs["launch"][1].items():
        if "tracked" in k:
            assert int(v) == int(before[k]) + 1 and int(outs["composed"][1][k]) == int(v)
        else:
            assert not torch.equal(v, before[k])
            assert float((v - outs["composed"][1][k]).abs().max()) <= 1e-4 * float(v.abs().max()), k
