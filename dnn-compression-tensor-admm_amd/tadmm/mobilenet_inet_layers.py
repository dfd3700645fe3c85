"""The ImageNet MobileNetV2 of the reference's main path (mobilenetv2_tt.py: _make_divisible, TTInvertedResidual,
TTMobileNetV2 and the `ttr_` / `tkc_` / `svdc_` / `svdm_mobilenetv2` factories), without timm.  State-dict keys
(`features.0.{0,1}`, `features.k.conv.j` with the reference's two Sequential layouts -- depthwise 0, BatchNorm 1, linear 3,
BatchNorm 4 for expansion 1; pointwise 0, BatchNorm 1, depthwise 3, BatchNorm 4, linear 6, BatchNorm 7 otherwise --
`conv.0`, `conv.1`, `classifier`), initialisation, `width_mult` and `cfgs` are the reference's; the modules that own
parameters stay nn.Conv2d and nn.BatchNorm2d.

Inside a block the depthwise stage goes through `functional.depthwise_bn_relu6` (csrc/dwbn.hip) and the linear
bottleneck, with the identity where the block has one, through `functional.batch_norm_act(relu=False, residual=...)`
(csrc/bnact.hip); the pointwise expansion, the stem and the head keep torch's batch norm and ReLU6.  A 1x1 convolution is
factorised exactly when its name is in `hp_dict.ranks`.

Reproduced from the reference: `tt_mobilenetv2_hp` keys its ranks `features.2.conv.0.0.weight` ... and
`tk_mobilenetv2_hp` `blocks.1.0.conv_pw.weight` ..., while this file asks for `features.2.conv.0.weight` ...; only
`svd_mobilenetv2_hp` matches.  `ttr_mobilenetv2` and `tkc_mobilenetv2` with their own tables therefore build an all-dense
network, there and here; names are not mapped.
Deviations: a table that lists a depthwise kernel is refused with a ValueError (the reference would hand `groups` to a
factorised class, which raises there too); `decompose=True, pretrained=True`, where the reference downloads timm's
`mobilenetv2_100`, wants `dense_dict=` or a local `path`: nothing is downloaded."""
import math
from functools import partial

import torch.nn as nn

from . import functional as HF
from .svd_layers import SVDConv2dC, SVDConv2dM
from .tk_layers import TKConv2dC
from .tt_layers import TTConv2dR
from ._layer_common import create_model


def _make_divisible(v, divisor, min_value=None):
    """Rounds v to a multiple of divisor, not below min_value and not more than 10 % below v (the original tf rule)."""
    if min_value is None:
        min_value = divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def conv_3x3_bn(inp, oup, stride):
    return nn.Sequential(nn.Conv2d(inp, oup, 3, stride, 1, bias=False), nn.BatchNorm2d(oup), nn.ReLU6(inplace=True))


def conv_1x1_bn(inp, oup):
    return nn.Sequential(nn.Conv2d(inp, oup, 1, 1, 0, bias=False), nn.BatchNorm2d(oup), nn.ReLU6(inplace=True))


def tt_conv_1x1_bn(inp, oup, conv, hp_dict, name, dense_w):
    return nn.Sequential(conv(inp, oup, 1, 1, 0, bias=False, hp_dict=hp_dict, name=name, dense_w=dense_w),
                         nn.BatchNorm2d(oup), nn.ReLU6(inplace=True))


def _pointwise(conv, hp_dict, dense_dict, w_name, inp, oup):
    if hp_dict is not None and w_name in hp_dict.ranks:
        return conv(inp, oup, 1, 1, 0, bias=False, hp_dict=hp_dict, name=w_name,
                    dense_w=None if dense_dict is None else dense_dict[w_name])
    return nn.Conv2d(inp, oup, 1, 1, 0, bias=False)


def _depthwise(hp_dict, w_name, dim, stride):
    if hp_dict is not None and w_name in hp_dict.ranks:
        raise ValueError(f"{w_name} is a depthwise kernel: the factorised layers take groups = 1 only, and no shipped rank "
                         "table lists it")
    return nn.Conv2d(dim, dim, 3, stride, 1, groups=dim, bias=False)


class TTInvertedResidual(nn.Module):
    def __init__(self, inp, oup, stride, expand_ratio, id=None, conv=TTConv2dR, hp_dict=None, dense_dict=None):
        super().__init__()
        assert stride in [1, 2]
        hidden_dim = round(inp * expand_ratio)
        self.identity = stride == 1 and inp == oup
        pre = 'features.' + str(id) + '.conv.'
        if expand_ratio == 1:
            layers = [_depthwise(hp_dict, pre + '0.weight', hidden_dim, stride), nn.BatchNorm2d(hidden_dim),
                      nn.ReLU6(inplace=True),
                      _pointwise(conv, hp_dict, dense_dict, pre + '3.weight', hidden_dim, oup), nn.BatchNorm2d(oup)]
        else:
            layers = [_pointwise(conv, hp_dict, dense_dict, pre + '0.weight', inp, hidden_dim), nn.BatchNorm2d(hidden_dim),
                      nn.ReLU6(inplace=True),
                      _depthwise(hp_dict, pre + '3.weight', hidden_dim, stride), nn.BatchNorm2d(hidden_dim),
                      nn.ReLU6(inplace=True),
                      _pointwise(conv, hp_dict, dense_dict, pre + '6.weight', hidden_dim, oup), nn.BatchNorm2d(oup)]
        self.expanded = expand_ratio != 1
        self.conv = nn.Sequential(*layers)
        self.route = None                       # None: the measured rules; "launch" / "composed" force a route

    def set_route(self, route):
        self.route = route
        return self

    def forward(self, x):
        m, out, k = self.conv, x, 0
        if self.expanded:
            out, k = m[2](m[1](m[0](x))), 3
        out = HF.depthwise_bn_relu6_module(m[k], m[k + 1], out, route=self.route)
        return HF.batch_norm_act_module(m[k + 4], m[k + 3](out), x if self.identity else None, relu=False,
                                        route=self.route)


class TTMobileNetV2(nn.Module):
    def __init__(self, num_classes=1000, width_mult=1., cfgs=None, conv=TTConv2dR, hp_dict=None, dense_dict=None):
        super().__init__()
        # t, c, n, s
        self.cfgs = [[1, 16, 1, 1], [6, 24, 2, 2], [6, 32, 3, 2], [6, 64, 4, 2], [6, 96, 3, 1], [6, 160, 3, 2],
                     [6, 320, 1, 1]] if cfgs is None else cfgs
        div = 4 if width_mult == 0.1 else 8
        input_channel = _make_divisible(32 * width_mult, div)
        layers = [conv_3x3_bn(3, input_channel, 2)]
        id = 1
        for t, c, n, s in self.cfgs:
            output_channel = _make_divisible(c * width_mult, div)
            for i in range(n):
                layers.append(TTInvertedResidual(input_channel, output_channel, s if i == 0 else 1, t, id=id, conv=conv,
                                                 hp_dict=hp_dict, dense_dict=dense_dict))
                input_channel = output_channel
                id += 1
        self.features = nn.Sequential(*layers)
        output_channel = _make_divisible(1280 * width_mult, div) if width_mult > 1.0 else 1280
        w_name = 'conv.0.weight'
        if hp_dict is not None and w_name in hp_dict.ranks:
            self.conv = tt_conv_1x1_bn(input_channel, output_channel, conv=conv, hp_dict=hp_dict, name=w_name,
                                       dense_w=None if dense_dict is None else dense_dict[w_name])
        else:
            self.conv = conv_1x1_bn(input_channel, output_channel)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.classifier = nn.Linear(output_channel, num_classes)
        self.route = None
        self._initialize_weights()

    def set_route(self, route):
        """Forces one route (None, "launch", "composed") on the depthwise stage and the bottleneck tail of every block;
        returns self."""
        self.route = route
        for m in self.features:
            if isinstance(m, TTInvertedResidual):
                m.set_route(route)
        return self

    def forward(self, x):
        x = self.features(x)
        x = self.conv(x)
        x = self.avgpool(x)
        return self.classifier(x.view(x.size(0), -1))

    def _initialize_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
                if m.bias is not None:
                    m.bias.data.zero_()
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()
            elif isinstance(m, nn.Linear):
                m.weight.data.normal_(0, 0.01)
                m.bias.data.zero_()


def _tt_mobilenetv2(conv, hp_dict, dense_dict=None, **kwargs):
    model = TTMobileNetV2(conv=conv, hp_dict=hp_dict, dense_dict=dense_dict, **kwargs)
    if dense_dict is not None:                  # the dense parts take the dense model's values
        tt_dict = model.state_dict()
        for key in tt_dict:
            if key in dense_dict:
                tt_dict[key] = dense_dict[key]
        model.load_state_dict(tt_dict)
    return model


def _factory(name, conv):
    def create(hp_dict, decompose=False, pretrained=False, path=None, dense_dict=None, **kwargs):
        if decompose and dense_dict is None and pretrained and path is None:
            raise ValueError(f"{name}(decompose=True, pretrained=True): the reference downloads timm's "
                             "mobilenetv2_100 here; nothing is downloaded -- give the dense state dict as "
                             "dense_dict= or a local file as path=")
        return create_model(name, partial(_tt_mobilenetv2, conv=conv, **kwargs), hp_dict, decompose, pretrained, path,
                            dense_dict)
    create.__name__ = create.__qualname__ = name
    create.__doc__ = (f"mobilenetv2_tt.py: {name}(hp_dict, decompose=False, pretrained=False, path=None, dense_dict=None, "
                      "**kwargs).  decompose=True factorises the dense state dict given as dense_dict= (or saved at the "
                      "local `path`); pretrained=True without decompose loads a compressed state dict from the local `path`.")
    return create


_CONV = {"ttr": TTConv2dR, "tkc": TKConv2dC, "svdc": SVDConv2dC, "svdm": SVDConv2dM}
FACTORIES = tuple(f"{kind}_mobilenetv2" for kind in _CONV)
for _kind, _cls in _CONV.items():
    globals()[f"{_kind}_mobilenetv2"] = _factory(f"{_kind}_mobilenetv2", _cls)
del _kind, _cls

__all__ = ["_make_divisible", "conv_3x3_bn", "conv_1x1_bn", "tt_conv_1x1_bn", "TTInvertedResidual", "TTMobileNetV2",
           "FACTORIES"] + list(FACTORIES)
