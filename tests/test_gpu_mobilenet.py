"""tadmm/mobilenet_cifar_layers.py and mobilenet_inet_layers.py on the device, float32: blocks and whole models with the
depthwise stage (csrc/dwbn.hip) and the bottleneck tail (csrc/bnact.hip) forced to the launch, against the float64
restatement of tests/_mobilenet_ref.py; the composed routes are the yardstick under the rule of tests/test_gpu_resnet.py,
in the max norm: with e_f the launch route's error and e_c the composed route's, both max |err| / max |float64 value|,
e_f <= 2 max(e_c, 2^-23), for the output and every parameter gradient.  The factorised 1x1 convolutions are restated too:
their dense kernels are the SVD factors multiplied out in float64, and float64 autograd carries the gradients to the
factors."""
import pytest
import torch

import _mobilenet_ref as R
from test_gpu_resnet import bar, both_routes, randomise, rel
from tadmm import get_hp_dict
from tadmm import mobilenet_cifar_layers as MC
from tadmm import mobilenet_inet_layers as MI

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


class NoRanks:
    ranks = {}


def cifar_block(which):
    hp = get_hp_dict("svdc_mobilenetv2_cifar", "2")
    MC.TTBaseBlock.alpha = 1
    if which == "id6":                                 # 32 -> 64, downsample, no shortcut
        return MC.TTBaseBlock(32, 64, downsample=True, conv=MC.SVDConv2dC, id=6, hp_dict=hp), 32
    if which == "id4":                                 # 32 -> 32, shortcut
        return MC.TTBaseBlock(32, 32, conv=MC.SVDConv2dC, id=4, hp_dict=hp), 32
    return MC.TTBaseBlock(16, 16, conv=MC.SVDConv2dC, id=2, hp_dict=NoRanks), 16


@pytest.mark.parametrize("which", ["id6", "id4", "dense"])
def test_cifar_block_against_float64(which):
    """mobilenetv2_cifar_tt.py: TTBaseBlock 6 and 4 from the svd table and one dense block, on a (2, C, 8, 8) input."""
    torch.manual_seed(21)
    blk, c = cifar_block(which)
    blk = randomise(blk, 2).to(DEV)
    assert isinstance(blk.conv3, MC.SVDConv2dC) == (which != "dense") and isinstance(blk.conv2, torch.nn.Conv2d)
    assert blk.shortcut == (which != "id6") and blk.stride == (2 if which == "id6" else 1)
    x = torch.randn(2, c, 8, 8)
    both_routes(blk, lambda x64, sd, tr: R.cifar_block(x64, sd, "", blk, tr), x, True, f"cifar block {which}")


@pytest.mark.parametrize("which", ["t1", "t6s2"])
def test_inet_block_against_float64(which):
    """mobilenetv2_tt.py: TTInvertedResidual with expansion 1 (features.1) and with expansion 6 at stride 2 (features.4,
    from the svd table), on a (2, C, 7, 7) input."""
    torch.manual_seed(22)
    hp = get_hp_dict("svdm_mobilenetv2", "2")
    if which == "t1":
        blk, c = MI.TTInvertedResidual(32, 16, 1, 1, id=1, conv=MI.SVDConv2dM, hp_dict=hp), 32
    else:
        blk, c = MI.TTInvertedResidual(24, 32, 2, 6, id=4, conv=MI.SVDConv2dM, hp_dict=hp), 24
        assert isinstance(blk.conv[0], MI.SVDConv2dM) and isinstance(blk.conv[6], MI.SVDConv2dM)
    blk = randomise(blk, 3).to(DEV)
    assert not blk.identity and blk.expanded == (which != "t1")
    x = torch.randn(2, c, 7, 7)
    both_routes(blk, lambda x64, sd, tr: R.inet_block(x64, sd, "", blk, tr), x, True, f"inet block {which}")


@pytest.mark.parametrize("case", [("svdc_mobilenetv2_cifar", MC, (2, 3, 32, 32)), ("svdm_mobilenetv2", MI, (2, 3, 64, 64))],
                         ids=lambda c: c[0])
def test_whole_model_training_step_and_eval_forward(case):
    name, mod, shape = case
    torch.manual_seed(23)
    model = randomise(getattr(mod, name)(get_hp_dict(name, "2"), num_classes=10), 4).to(DEV)
    ref_fn = R.cifar_mobilenet if mod is MC else R.inet_mobilenet
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


def test_svdr_cifar_constructs_from_a_dense_state_dict():
    """`svdr_mobilenetv2_cifar` with the shipped table builds only from a dense weight (SVDConv2dR's own initialisation
    multiplies (r, I) by (O, r), as the reference's): decompose=True with a dense state dict, whose SVD runs on the
    device."""
    torch.manual_seed(24)
    dense = MC.tkc_mobilenetv2_cifar(NoRanks).to(DEV).state_dict()
    model = MC.svdr_mobilenetv2_cifar(get_hp_dict("svdr_mobilenetv2_cifar", "2"), decompose=True, dense_dict=dense).to(DEV)
    assert isinstance(model.bottlenecks[3].conv1, MC.SVDConv2dR) and isinstance(model.bottlenecks[3].conv2, torch.nn.Conv2d)
    assert torch.equal(model.bottlenecks[3].conv2.weight, dense["bottlenecks.3.conv2.weight"])
    with torch.no_grad():
        out = model.eval()(torch.randn(2, 3, 32, 32, device=DEV))
    assert out.shape == (2, 10) and bool(torch.isfinite(out).all())
