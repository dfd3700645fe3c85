"""The CIFAR MobileNetV2 of the reference's main path (mobilenetv2_cifar_tt.py: TTBaseBlock, TTMobileNetV2 and the
`tkr_` / `tkc_` / `tkm_` / `svdr_` / `svdc_` / `svdm_mobilenetv2_cifar` factories), without timm.  State-dict keys
(`conv0`, `bn0`, `bottlenecks.i.{conv1,bn1,conv2,bn2,conv3,bn3}`, `conv1`, `bn1`, `fc`), initialisation, the class-level
`alpha` and the constructor arguments are the reference's, so a dense `mobilenetv2_cifar` checkpoint decomposes and a
compressed one loads as they do there; the modules that own parameters stay nn.Conv2d and nn.BatchNorm2d.

Inside a block the depthwise stage relu6(bn2(conv2(x))) goes through `functional.depthwise_bn_relu6` (csrc/dwbn.hip)
and the linear bottleneck bn3(conv3(x)) [+ inputs] through `functional.batch_norm_act(relu=False, residual=...)`
(csrc/bnact.hip).  The pointwise relu6(bn1(conv1(x))) and the stem stay torch's batch norm and `F.relu6`: their upper
clamp is not in bnact.hip.  `conv` builds the 1x1 convolutions whose weight name is in `hp_dict.ranks`; the others are
nn.Conv2d.  Nothing is ever downloaded: a dense state dict comes from `dense_dict=` or a local file.

Deviation: no shipped table lists a depthwise kernel (`bottlenecks.i.conv2.weight`), and the reference builds conv2 as
nn.Conv2d whatever the table says; a table that lists one is refused here with a ValueError instead of being ignored."""
import math
from functools import partial

import torch.nn as nn
import torch.nn.functional as F

from . import functional as HF
from .svd_layers import SVDConv2dC, SVDConv2dM, SVDConv2dR
from .tk_layers import TKConv2dC, TKConv2dM, TKConv2dR
from ._layer_common import create_model


def _pointwise(conv, hp_dict, dense_dict, w_name, inp, oup):
    if hp_dict is not None and w_name in hp_dict.ranks:
        return conv(inp, oup, kernel_size=1, bias=False, hp_dict=hp_dict, name=w_name,
                    dense_w=None if dense_dict is None else dense_dict[w_name])
    return nn.Conv2d(inp, oup, kernel_size=1, bias=False)


class TTBaseBlock(nn.Module):
    alpha = 1

    def __init__(self, input_channel, output_channel, t=6, downsample=False, conv=TKConv2dC, id=None, hp_dict=None,
                 dense_dict=None):
        """t: expansion factor, t * input_channel is the width of the expansion layer; the class attribute alpha is the
        width multiplier."""
        super().__init__()
        self.stride = 2 if downsample else 1
        self.downsample = downsample
        self.shortcut = (not downsample) and (input_channel == output_channel)
        input_channel = int(self.alpha * input_channel)
        output_channel = int(self.alpha * output_channel)
        c = t * input_channel
        pre = 'bottlenecks.' + str(id)
        if hp_dict is not None and pre + '.conv2.weight' in hp_dict.ranks:
            raise ValueError(f"{pre}.conv2.weight is a depthwise kernel: the factorised layers take groups = 1 only, and "
                             "no shipped rank table lists it")
        self.conv1 = _pointwise(conv, hp_dict, dense_dict, pre + '.conv1.weight', input_channel, c)
        self.bn1 = nn.BatchNorm2d(c)
        self.conv2 = nn.Conv2d(c, c, kernel_size=3, stride=self.stride, padding=1, groups=c, bias=False)
        self.bn2 = nn.BatchNorm2d(c)
        self.conv3 = _pointwise(conv, hp_dict, dense_dict, pre + '.conv3.weight', c, output_channel)
        self.bn3 = nn.BatchNorm2d(output_channel)
        self.route = None                       # None: the measured rules; "launch" / "composed" force a route

    def set_route(self, route):
        self.route = route
        return self

    def forward(self, inputs):
        x = F.relu6(self.bn1(self.conv1(inputs)))
        x = HF.depthwise_bn_relu6_module(self.conv2, self.bn2, x, route=self.route)
        return HF.batch_norm_act_module(self.bn3, self.conv3(x), inputs if self.shortcut else None, relu=False,
                                        route=self.route)


class TTMobileNetV2(nn.Module):
    def __init__(self, output_size=10, alpha=1, conv=TKConv2dC, hp_dict=None, dense_dict=None):
        super().__init__()
        self.output_size = output_size
        self.conv0 = nn.Conv2d(3, int(32 * alpha), kernel_size=3, stride=1, padding=1, bias=False)
        self.bn0 = nn.BatchNorm2d(int(32 * alpha))
        TTBaseBlock.alpha = alpha
        kw = dict(conv=conv, hp_dict=hp_dict, dense_dict=dense_dict)
        # (input, output, t or None for the default 6, downsample or None for the default)
        cfg = [(32, 16, 1, False), (16, 24, None, False), (24, 24, None, None), (24, 32, None, False), (32, 32, None, None),
               (32, 32, None, None), (32, 64, None, True), (64, 64, None, None), (64, 64, None, None), (64, 64, None, None),
               (64, 96, None, False), (96, 96, None, None), (96, 96, None, None), (96, 160, None, True),
               (160, 160, None, None), (160, 160, None, None), (160, 320, None, False)]
        self.bottlenecks = nn.Sequential(*[
            TTBaseBlock(i, o, **({} if t is None else {"t": t}), **({} if d is None else {"downsample": d}), id=k, **kw)
            for k, (i, o, t, d) in enumerate(cfg)])
        self.conv1 = _pointwise(conv, hp_dict, dense_dict, 'conv1.weight', int(320 * alpha), 1280)
        self.bn1 = nn.BatchNorm2d(1280)
        self.fc = nn.Linear(1280, output_size)
        self.route = None
        self.weights_init()

    def weights_init(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()

    def set_route(self, route):
        """Forces one route (None, "launch", "composed") on the depthwise stage and the bottleneck tail of every block;
        returns self."""
        self.route = route
        for m in self.bottlenecks:
            m.set_route(route)
        return self

    def forward(self, inputs):
        x = F.relu6(self.bn0(self.conv0(inputs)))
        x = self.bottlenecks(x)
        x = F.relu6(self.bn1(self.conv1(x)))
        x = F.adaptive_avg_pool2d(x, 1)
        return self.fc(x.view(x.shape[0], -1))


def _tt_mobilenetv2_cifar(num_classes=10, conv=TKConv2dC, hp_dict=None, dense_dict=None, **kwargs):
    if 'num_classes' in kwargs:
        num_classes = kwargs.get('num_classes')
    model = TTMobileNetV2(output_size=num_classes, conv=conv, hp_dict=hp_dict, dense_dict=dense_dict)
    if dense_dict is not None:                  # the dense parts take the dense model's values
        tk_dict = model.state_dict()
        for key in tk_dict:
            if key in dense_dict:
                tk_dict[key] = dense_dict[key]
        model.load_state_dict(tk_dict)
    return model


def _factory(name, conv, always):
    def create(hp_dict, decompose=False, pretrained=False, path=None, dense_dict=None, **kwargs):
        return create_model(name, partial(_tt_mobilenetv2_cifar, conv=conv, **kwargs), hp_dict, decompose, pretrained,
                            path, dense_dict, load_with_decompose=always)
    create.__name__ = create.__qualname__ = name
    create.__doc__ = (f"mobilenetv2_cifar_tt.py: {name}(hp_dict, decompose=False, pretrained=False, path=None, "
                      "dense_dict=None, **kwargs).  decompose=True factorises the dense state dict given as dense_dict= (or "
                      "saved at the local `path`); pretrained=True loads a compressed state dict from the local `path`.")
    return create


# tkr_ loads `path` under pretrained even with decompose, as the reference does; the others only without
_CONV = {"tkr": TKConv2dR, "tkc": TKConv2dC, "tkm": TKConv2dM, "svdr": SVDConv2dR, "svdc": SVDConv2dC, "svdm": SVDConv2dM}
FACTORIES = tuple(f"{kind}_mobilenetv2_cifar" for kind in _CONV)
for _kind, _cls in _CONV.items():
    globals()[f"{_kind}_mobilenetv2_cifar"] = _factory(f"{_kind}_mobilenetv2_cifar", _cls, _kind == "tkr")
del _kind, _cls

__all__ = ["TTBaseBlock", "TTMobileNetV2", "FACTORIES"] + list(FACTORIES)
