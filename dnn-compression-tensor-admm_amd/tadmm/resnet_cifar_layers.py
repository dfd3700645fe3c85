"""The CIFAR ResNets of the reference's main path (resnet_cifar_tt.py: LambdaLayer, TTBasicBlock with the option-A and
option-B shortcuts, TTResNet and the `ttr_` / `ttm_` / `tkr_` / `tkm_` / `tkc_` / `stftkc_` factories), without timm.
State-dict keys, initialisation and constructor arguments are the reference's, so a `resnet32` checkpoint decomposes and
a compressed one loads as they do there; the BatchNorm modules stay nn.BatchNorm2d.

Every BatchNorm call with what follows it -- relu(bn1(conv1(x))) and relu(bn2(conv2(.)) + shortcut(x)) -- goes through
`functional.batch_norm_act` (csrc/bnact.hip).  The option-A shortcut hands the strided view x[:, :, ::2, ::2] and the
channel offset planes // 4 to the tail: neither the slice copy nor the zero padding of `F.pad` is materialised, and the
shortcut's gradient reaches the block input through autograd of that view.  `conv` is one of TTConv2dR / TTConv2dM /
TKConv2dC / TKConv2dM / TKConv2dR / StfTKConv2dC and builds the convolutions whose weight name is in `hp_dict.ranks`;
the others are nn.Conv2d.  Nothing is ever downloaded: a dense state dict comes from `dense_dict=` or a local file.

Deliberate deviation: the reference's `TTBasicBlock.forward_flops` feeds the block input, not conv1's output, to a dense
conv2 and counts conv2's weights for a dense conv1 (resnet_cifar_tt.py:112-125); here each convolution is fed and
counted as itself."""
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.nn.init as init

from . import functional as HF
from .stf_layers import StfTKConv2dC
from .tk_layers import TKConv2dC, TKConv2dM, TKConv2dR
from .tt_layers import TTConv2dM, TTConv2dR
from ._layer_common import create_model

_FLOPS_LAYERS = (TKConv2dC, TKConv2dM, TKConv2dR, TTConv2dM, TTConv2dR)


def _weights_init(m):
    if isinstance(m, (nn.Linear, nn.Conv2d)):
        init.kaiming_normal_(m.weight)


class LambdaLayer(nn.Module):
    def __init__(self, lambd):
        super().__init__()
        self.lambd = lambd

    def forward(self, x):
        return self.lambd(x)


def _conv(conv, hp_dict, dense_dict, w_name, in_planes, planes, kernel_size, stride, padding):
    if hp_dict is not None and w_name in hp_dict.ranks:
        return conv(in_planes, planes, kernel_size, stride=stride, padding=padding, bias=False, hp_dict=hp_dict,
                    name=w_name, dense_w=None if dense_dict is None else dense_dict[w_name])
    return nn.Conv2d(in_planes, planes, kernel_size, stride=stride, padding=padding, bias=False)


def _conv_flops(conv, x):
    """(output, dense MFLOPs, compressed MFLOPs) of one convolution, as the reference's forward_flops counts them."""
    if isinstance(conv, _FLOPS_LAYERS):
        return conv.forward_flops(x)
    out = conv(x)
    flops = out.shape[2] * out.shape[3] * conv.weight.numel() / 1000 / 1000
    return out, flops, flops


class TTBasicBlock(nn.Module):
    expansion = 1

    def __init__(self, in_planes, planes, stride=1, option='A', conv=TTConv2dR, stage=None, id=None, hp_dict=None,
                 dense_dict=None):
        super().__init__()
        pre = 'layer' + str(stage) + '.' + str(id)
        self.conv1 = _conv(conv, hp_dict, dense_dict, pre + '.conv1.weight', in_planes, planes, 3, stride, 1)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = _conv(conv, hp_dict, dense_dict, pre + '.conv2.weight', planes, planes, 3, 1, 1)
        self.bn2 = nn.BatchNorm2d(planes)
        self.shortcut = nn.Sequential()
        self.pad = None                         # option A: the channel offset of the strided view
        if stride != 1 or in_planes != planes:
            if option == 'A':                   # the CIFAR-10 ResNet paper's shortcut
                self.shortcut = LambdaLayer(lambda x: F.pad(x[:, :, ::2, ::2], (0, 0, 0, 0, planes // 4, planes // 4),
                                                            "constant", 0))
                if in_planes + 2 * (planes // 4) == planes:
                    self.pad = planes // 4
            elif option == 'B':
                self.shortcut = nn.Sequential(
                    nn.Conv2d(in_planes, self.expansion * planes, kernel_size=1, stride=stride, bias=False),
                    nn.BatchNorm2d(self.expansion * planes))
        self.route = None                       # None: the measured rule; "launch" / "composed" force a route

    def set_route(self, route):
        self.route = route
        return self

    def _tail(self, out, x):
        """relu(bn2(out) + shortcut(x))"""
        if self.pad is not None:
            return HF.batch_norm_act_module(self.bn2, out, x[:, :, ::2, ::2], self.pad, route=self.route)
        if isinstance(self.shortcut, nn.Sequential) and len(self.shortcut) == 2:
            res = HF.batch_norm_act_module(self.shortcut[1], self.shortcut[0](x), relu=False, route=self.route)
        else:
            res = self.shortcut(x)
        return HF.batch_norm_act_module(self.bn2, out, res, route=self.route)

    def forward(self, x):
        out = HF.batch_norm_act_module(self.bn1, self.conv1(x), route=self.route)
        return self._tail(self.conv2(out), x)

    def forward_features(self, x, name, features):
        out, f = self.conv1.forward_features(x)
        features[name + 'conv1'] = f
        out = HF.batch_norm_act_module(self.bn1, out, route=self.route)
        out, f = self.conv2.forward_features(out)
        features[name + 'conv2'] = f
        return self._tail(out, x)

    def forward_flops(self, x, name):
        print('>{}:\t'.format(name + 'conv1'), end='', flush=True)
        out, base1, compr1 = _conv_flops(self.conv1, x)
        out = HF.batch_norm_act_module(self.bn1, out, route=self.route)
        print('>{}:\t'.format(name + 'conv2'), end='', flush=True)
        out, base2, compr2 = _conv_flops(self.conv2, out)
        return self._tail(out, x), base1 + base2, compr1 + compr2


class TTResNet(nn.Module):
    def __init__(self, num_blocks, num_classes=10, conv=TTConv2dR, hp_dict=None, dense_dict=None):
        super().__init__()
        self.in_planes = 16
        self.conv1 = nn.Conv2d(3, 16, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(16)
        self.layer1 = self._make_layer(TTBasicBlock, 16, num_blocks[0], stride=1, stage=1, conv=conv, hp_dict=hp_dict,
                                       dense_dict=dense_dict)
        self.layer2 = self._make_layer(TTBasicBlock, 32, num_blocks[1], stride=2, stage=2, conv=conv, hp_dict=hp_dict,
                                       dense_dict=dense_dict)
        self.layer3 = self._make_layer(TTBasicBlock, 64, num_blocks[2], stride=2, stage=3, conv=conv, hp_dict=hp_dict,
                                       dense_dict=dense_dict)
        self.linear = nn.Linear(64, num_classes)
        self.route = None
        self.apply(_weights_init)

    def _make_layer(self, block, planes, num_blocks, stride, stage, conv, hp_dict=None, dense_dict=None):
        layers = []
        for id, stride in enumerate([stride] + [1] * (num_blocks - 1)):
            layers.append(block(self.in_planes, planes, stride, stage=stage, id=id, conv=conv, hp_dict=hp_dict,
                                dense_dict=dense_dict))
            self.in_planes = planes * block.expansion
        return nn.Sequential(*layers)

    def set_route(self, route):
        """Forces one route (None, "launch", "composed") on every BatchNorm tail; returns self."""
        self.route = route
        for m in self.modules():
            if isinstance(m, TTBasicBlock):
                m.set_route(route)
        return self

    def _stages(self):
        for s, layer in enumerate((self.layer1, self.layer2, self.layer3), 1):
            for i, block in enumerate(layer):
                yield 'layer{}.{}.'.format(s, i), block

    def _stem(self, x):
        return HF.batch_norm_act_module(self.bn1, self.conv1(x), route=self.route)

    def _head(self, out):
        out = F.avg_pool2d(out, out.size()[3])
        return self.linear(out.view(out.size(0), -1))

    def forward(self, x):
        out = self._stem(x)
        out = self.layer1(out)
        out = self.layer2(out)
        out = self.layer3(out)
        return self._head(out)

    def forward_features(self, x):
        features = {}
        out = self._stem(x)
        for name, block in self._stages():
            out = block.forward_features(out, name, features)
        return self._head(out), features

    def forward_flops(self, x):
        base_flops = compr_flops = 0
        out = self._stem(x)
        for name, block in self._stages():
            out, flops1, flops2 = block.forward_flops(out, name)
            base_flops += flops1
            compr_flops += flops2
        return self._head(out), base_flops, compr_flops


def _tt_resnet(num_blocks, num_classes=10, conv=TTConv2dR, hp_dict=None, dense_dict=None, **kwargs):
    if 'num_classes' in kwargs:
        num_classes = kwargs.get('num_classes')
    model = TTResNet(num_blocks, num_classes=num_classes, conv=conv, hp_dict=hp_dict, dense_dict=dense_dict)
    if dense_dict is not None:                  # the dense parts take the dense model's values
        tt_dict = model.state_dict()
        for key in tt_dict:
            if key in dense_dict:
                tt_dict[key] = dense_dict[key]
        model.load_state_dict(tt_dict)
    return model


def _factory(name, conv, num_blocks):
    def create(hp_dict, decompose=False, pretrained=False, path=None, dense_dict=None, **kwargs):
        # as the reference does, pretrained loads `path` even behind decompose
        return create_model(name, partial(_tt_resnet, num_blocks, conv=conv, **kwargs), hp_dict, decompose, pretrained,
                            path, dense_dict, load_with_decompose=True)
    create.__name__ = create.__qualname__ = name
    create.__doc__ = (f"resnet_cifar_tt.py: {name}(hp_dict, decompose=False, pretrained=False, path=None, dense_dict=None, "
                      "**kwargs).  decompose=True factorises the dense state dict given as dense_dict= (or saved at the "
                      "local `path`); pretrained=True loads a compressed state dict from the local `path`.")
    return create


_BLOCKS = {"resnet20": [3, 3, 3], "resnet32": [5, 5, 5], "resnet56": [9, 9, 9]}
# the thirteen the reference defines: no ttm_ / tkm_ / tkc_resnet56 there
_DEFINED = {"ttr": (TTConv2dR, ("resnet32", "resnet20", "resnet56")), "ttm": (TTConv2dM, ("resnet32", "resnet20")),
            "tkr": (TKConv2dR, ("resnet32", "resnet20", "resnet56")), "tkm": (TKConv2dM, ("resnet32", "resnet20")),
            "tkc": (TKConv2dC, ("resnet32", "resnet20")), "stftkc": (StfTKConv2dC, ("resnet32",))}
FACTORIES = tuple(f"{kind}_{arch}" for kind, (_, archs) in _DEFINED.items() for arch in archs)
for _kind, (_cls, _archs) in _DEFINED.items():
    for _arch in _archs:
        globals()[f"{_kind}_{_arch}"] = _factory(f"{_kind}_{_arch}", _cls, _BLOCKS[_arch])
del _kind, _cls, _archs, _arch

__all__ = ["LambdaLayer", "TTBasicBlock", "TTResNet", "FACTORIES"] + list(FACTORIES)
