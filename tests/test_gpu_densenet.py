"""tadmm/densenet_cifar_layers.py and densenet_inet_layers.py on the device, float32: blocks, transitions and whole models
with every BatchNorm forced to the launch (csrc/densebn.hip for the lists of feature tensors, csrc/bnact.hip for single
tensors), against the float64 restatement of tests/_densenet_ref.py; the composed route is the yardstick under the rule
of tests/test_gpu_resnet.py, in the max norm: with e_f the launch route's error and e_c the composed route's, both
max |err| / max |float64 value|, e_f <= 2 max(e_c, 2^-23), for the output and every parameter gradient.  The factorised
convolutions are restated too: their dense kernels are the factors multiplied out in float64
(`_resnet_ref.dense_weight`), and float64 autograd carries the gradients to the factors."""
import pytest
import torch

import _densenet_ref as D
from tadmm import get_hp_dict
from tadmm import densenet_cifar_layers as DC
from tadmm import densenet_inet_layers as DI
from tadmm.functional import DenseFeatures

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -23


class NoRanks:
    ranks = {}
    tt_shapes = {}


def bar(e_f, e_c, what):
    print(f"    {what:<52s} launch {e_f:.3e}   composed {e_c:.3e}")
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


def tensor_of(out):
    return out.cat() if isinstance(out, DenseFeatures) else out


def both_routes(mod, ref_fn, x, training, what):
    """Output and every parameter gradient of `mod` (on the device) under both routes against `ref_fn(x64, sd, training)`."""
    mod.train(training)
    sd = D.state64(mod, requires_grad=True)
    names = [n for n, _ in mod.named_parameters()]
    want = ref_fn(D.f64(x), sd, training)
    up = torch.randn(want.shape, generator=torch.Generator().manual_seed(1))
    want_g = torch.autograd.grad(want, [sd[n] for n in names], D.f64(up))
    got = {}
    for route in ("launch", "composed"):
        out = tensor_of(mod.set_route(route)(x.to(DEV)))
        got[route] = [out] + list(torch.autograd.grad(out, list(mod.parameters()), up.to(DEV)))
    worst = 0.0
    for i, (key, ref) in enumerate(zip(["output"] + names, [want] + list(want_g))):
        worst = max(worst, bar(rel(got["launch"][i], ref), rel(got["composed"][i], ref), f"{what} {key}"))
    print(f"    worst launch error of {what}: {worst:.3e}")


@pytest.mark.parametrize("kind", ["dense", "tkr"])
def test_cifar_dense_block_against_float64(kind):
    """densenet_cifar_tt.py: TenDenseBlock of three basic layers on a (2, C, 8, 8) input.  dense: 8 channels in, growth
    4, nn.Conv2d.  tkr: the first three layers of block 1 of tkr_densenet40 (32 channels in, growth 16, TKConv2dR from
    the shipped table)."""
    torch.manual_seed(11)
    if kind == "dense":
        blk, cin = DC.TenDenseBlock(3, 8, 4, DC.TenBasicBlock, conv=DC.TKConv2dR, stage=1, hp_dict=NoRanks), 8
    else:
        blk, cin = DC.TenDenseBlock(3, 32, 16, DC.TenBasicBlock, conv=DC.TKConv2dR, stage=1,
                                    hp_dict=get_hp_dict("tkr_densenet40", "2")), 32
    blk = randomise(blk, 2).to(DEV)
    assert all(isinstance(layer.conv1, DC.TKConv2dR) == (kind == "tkr") for layer in blk.layer)
    x = torch.randn(2, cin, 8, 8)
    both_routes(blk, lambda x64, sd, tr: D.cifar_dense_block(x64, sd, "", blk, tr), x, True, f"{kind} cifar block")


def test_cifar_transition_against_float64():
    """densenet_cifar_tt.py: TenTransitionBlock 16 -> 8 on the three feature tensors (8, 4, 4 channels) of a block."""
    torch.manual_seed(12)
    trans = randomise(DC.TenTransitionBlock(16, 8, conv=DC.TKConv2dR, stage=1, hp_dict=NoRanks), 3).to(DEV)

    class OnList(torch.nn.Module):
        """The transition on a block's DenseFeatures: the input tensor cut into the block's segments."""

        def __init__(self):
            super().__init__()
            self.trans = trans

        def set_route(self, route):
            self.trans.set_route(route)
            return self

        def forward(self, x):
            return self.trans(DenseFeatures([x[:, :8].contiguous(), x[:, 8:12].contiguous(), x[:, 12:].contiguous()]))

    x = torch.randn(2, 16, 8, 8)
    both_routes(OnList(), lambda x64, sd, tr: D.cifar_transition(x64, sd, "trans.", trans, tr), x, True, "cifar transition")


@pytest.mark.parametrize("kind", ["dense", "tkc"])
def test_inet_dense_block_and_transition_against_float64(kind):
    """densenet_inet_tt.py: TenDenseBlock of two layers and the TenDenseTransition behind it on a (2, C, 7, 7) input.
    dense: 8 channels in, growth 4.  tkc: the first two layers of denseblock1 of tkc_densenet121 (64 in, growth 32, conv2
    a TKConv2dC from the shipped table) and a transition 128 -> 64 under a stage the table does not name (nn.Conv2d)."""
    torch.manual_seed(13)
    if kind == "dense":
        cin, grow, hp = 8, 4, NoRanks
    else:
        cin, grow, hp = 64, 32, get_hp_dict("tkc_densenet121", "2")

    class BlockAndTransition(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.denseblock1 = DI.TenDenseBlock(2, cin, 4, grow, stage=1, hp_dict=hp)
            self.transition9 = DI.TenDenseTransition(cin + 2 * grow, (cin + 2 * grow) // 2, stage=9, hp_dict=hp)

        def set_route(self, route):
            return DI.set_route(self, route)

        def forward(self, x):
            return self.transition9(self.denseblock1(x))

    mod = randomise(BlockAndTransition(), 4).to(DEV)
    assert isinstance(mod.denseblock1.denselayer1.conv2, DI.TKConv2dC) == (kind == "tkc")

    def ref(x64, sd, tr):
        out = D.inet_dense_block(x64, sd, "denseblock1.", mod.denseblock1, tr)
        return D.inet_transition(out, sd, "transition9.", mod.transition9, tr)

    x = torch.randn(2, cin, 7, 7)
    both_routes(mod, ref, x, True, f"{kind} inet block + transition")


def small_models():
    cifar = DC.TenDenseNet(10, num_classes=7, growth_rate=4, bottleneck=False, hp_dict=NoRanks)
    inet = DI.TenDenseNet(growth_rate=4, block_config=(2, 2), num_classes=5, hp_dict=NoRanks)
    return ((cifar, D.cifar_densenet, "cifar depth 10"), (inet, D.inet_densenet, "inet (2, 2)"))


@pytest.mark.parametrize("which", [0, 1], ids=["cifar", "inet"])
def test_small_whole_model_in_train_mode(which):
    """Depth 10 with growth 4 (CIFAR) and block_config (2, 2) with growth 4 (ImageNet), the models of the CPU test: logits
    and every parameter gradient; the buffers are updated alike on both routes."""
    torch.manual_seed(14)
    model, ref_fn, what = small_models()[which]
    model = randomise(model, 5).to(DEV)
    img = torch.randn(3, 3, 32, 32)
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "tracked" in k}
    both_routes(model, lambda x64, sd, tr: ref_fn(x64, sd, model, tr), img, True, what)
    after = {}
    for route in ("launch", "composed"):
        model.load_state_dict(before, strict=False)
        model.train().set_route(route)(img.to(DEV))
        after[route] = {k: v.clone() for k, v in model.state_dict().items() if k in before}
    for k, v in after["launch"].items():
        if "tracked" in k:
            assert int(v) == int(before[k]) + 1 and int(after["composed"][k]) == int(v), k
        else:
            assert not torch.equal(v, before[k])
            assert float((v - after["composed"][k]).abs().max()) <= 1e-4 * float(v.abs().max()), k


@pytest.mark.parametrize("which", [0, 1], ids=["cifar", "inet"])
def test_small_whole_model_in_eval_mode(which):
    torch.manual_seed(15)
    model, ref_fn, what = small_models()[which]
    model = randomise(model, 6).to(DEV).eval()
    img = torch.randn(3, 3, 32, 32)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    want = ref_fn(D.f64(img), D.state64(model), model, False)
    with torch.no_grad():
        got = {route: model.set_route(route)(img.to(DEV)) for route in ("launch", "composed")}
    assert got["launch"].shape == want.shape
    bar(rel(got["launch"], want), rel(got["composed"], want), f"{what} eval logits")
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())    # eval writes nothing
