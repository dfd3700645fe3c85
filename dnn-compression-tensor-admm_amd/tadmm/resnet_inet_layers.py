"""The ImageNet ResNets of the reference's main path (resnet_inet_tt.py: tt_conv3x3 / tt_conv1x1 with the one-rank ->
SVDConv2dC rule, TTBasicBlock, TTBottleneck, TTResNet with `zero_init_residual` and `forward_flops`, and the eleven
factories), without timm.  State-dict keys are torchvision's ResNet (conv1, bn1, layerS.I.convK / bnK / downsample.0 / .1,
fc) with the factorised layers' own keys in place of the replaced weights, the initialisation is the reference's, and the
BatchNorm modules stay nn.BatchNorm2d (or whatever `norm_layer` builds).

Every BatchNorm call with what follows it goes through `functional.batch_norm_act` (csrc/bnact.hip): relu(bn(conv(x)))
inside a block, relu(bn(conv(.)) + identity) at its end with the identity or the downsample's output as the residual,
and the downsample's own BatchNorm without ReLU.  `conv` is one of TTConv2dR / TTConv2dM / TKConv2dC / TKConv2dM /
TKConv2dR and builds the convolutions whose weight name is in `hp_dict.ranks`; the others are nn.Conv2d.  Nothing is ever
downloaded: where the reference fetches timm's pretrained dense model (`decompose=True, pretrained=True`), the dense
state dict comes from `dense_dict=` or a local file."""
from functools import partial

import torch
import torch.nn as nn

from . import functional as HF
from .svd_layers import SVDConv2dC, SVDConv2dM
from .tk_layers import TKConv2dC, TKConv2dM, TKConv2dR
from .tt_layers import TTConv2dM, TTConv2dR
from ._layer_common import create_model


def conv3x3(in_planes, out_planes, stride=1, groups=1, dilation=1):
    """3x3 convolution with padding"""
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=dilation, groups=groups, bias=False,
                     dilation=dilation)


def conv1x1(in_planes, out_planes, stride=1):
    """1x1 convolution"""
    return nn.Conv2d(in_planes, out_planes, kernel_size=1, stride=stride, bias=False)


def tt_conv3x3(in_planes, out_planes, stride=1, groups=1, dilation=1, conv=TTConv2dR, hp_dict=None, name=None,
               dense_w=None):
    """3x3 convolution with padding"""
    return conv(in_planes, out_planes, kernel_size=3, stride=stride, padding=dilation, groups=groups, bias=False,
                dilation=dilation, hp_dict=hp_dict, name=name, dense_w=dense_w)


def tt_conv1x1(in_planes, out_planes, stride=1, conv=TTConv2dR, hp_dict=None, name=None, dense_w=None):
    """1x1 convolution; a rank list of one entry is an SVD layer whatever `conv` is"""
    if len(hp_dict.ranks[name]) == 1:
        return SVDConv2dC(in_planes, out_planes, kernel_size=1, stride=stride, bias=False, hp_dict=hp_dict, name=name,
                          dense_w=dense_w)
    return conv(in_planes, out_planes, kernel_size=1, stride=stride, bias=False, hp_dict=hp_dict, name=name,
                dense_w=dense_w)


def _named(hp_dict, dense_dict, stage, id, which):
    """(weight name, whether the rank table has it, its dense weight) of layer<stage>.<id>.<which>"""
    w_name = 'layer' + str(stage) + '.' + str(id) + '.' + which + '.weight'
    listed = hp_dict is not None and w_name in hp_dict.ranks
    return w_name, listed, dense_dict[w_name] if listed and dense_dict is not None else None


def _conv_flops(conv, x, layers):
    """(output, dense MFLOPs, compressed MFLOPs) of one convolution, as the reference's forward_flops counts them."""
    if isinstance(conv, layers):
        return conv.forward_flops(x)
    out = conv(x)
    flops = out.shape[2] * out.shape[3] * conv.weight.numel() / 1000 / 1000
    return out, flops, flops


class _Routed(nn.Module):
    route = None                                # None: the measured rule; "launch" / "composed" force a route

    def set_route(self, route):
        self.route = route
        return self

    def _bn(self, bn, x, residual=None, relu=True):
        return HF.batch_norm_act_module(bn, x, residual, relu=relu, route=self.route)

    def _identity(self, x):
        """What the block's last tail adds: x, or the downsample's convolution behind its BatchNorm (no ReLU)."""
        ds = self.downsample
        if ds is None:
            return x
        if isinstance(ds, nn.Sequential) and len(ds) == 2:
            return self._bn(ds[1], ds[0](x), relu=False)
        return ds(x)


class TTBasicBlock(_Routed):
    expansion = 1
    _flops_layers = (TTConv2dM, TTConv2dR, TKConv2dC, TKConv2dM, TKConv2dR)

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64, dilation=1, norm_layer=None,
                 stage=1, id=0, conv=TTConv2dR, hp_dict=None, dense_dict=None):
        super().__init__()
        if norm_layer is None:
            norm_layer = nn.BatchNorm2d
        if groups != 1 or base_width != 64:
            raise ValueError('BasicBlock only supports groups=1 and base_width=64')
        if dilation > 1:
            raise NotImplementedError("Dilation > 1 not supported in BasicBlock")
        # both self.conv1 and self.downsample downsample the input when stride != 1
        w_name, listed, dense_w = _named(hp_dict, dense_dict, stage, id, 'conv1')
        self.conv1 = tt_conv3x3(inplanes, planes, stride, conv=conv, hp_dict=hp_dict, name=w_name, dense_w=dense_w) \
            if listed else conv3x3(inplanes, planes, stride)
        self.bn1 = norm_layer(planes)
        self.relu = nn.ReLU(inplace=True)
        w_name, listed, dense_w = _named(hp_dict, dense_dict, stage, id, 'conv2')
        self.conv2 = tt_conv3x3(planes, planes, conv=conv, hp_dict=hp_dict, name=w_name, dense_w=dense_w) \
            if listed else conv3x3(planes, planes)
        self.bn2 = norm_layer(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        out = self._bn(self.bn1, self.conv1(x))
        return self._bn(self.bn2, self.conv2(out), self._identity(x))

    def forward_flops(self, x, name):
        print('>{}:'.format(name + 'conv1'))
        out, base1, compr1 = _conv_flops(self.conv1, x, self._flops_layers)
        out = self._bn(self.bn1, out)
        print('>{}:'.format(name + 'conv2'))
        out, base2, compr2 = _conv_flops(self.conv2, out, self._flops_layers)
        return self._bn(self.bn2, out, self._identity(x)), base1 + base2, compr1 + compr2


class TTBottleneck(_Routed):
    # the stride sits at the 3x3 convolution (ResNet V1.5), as in torchvision
    expansion = 4
    _flops_layers = (TTConv2dM, TKConv2dC, TKConv2dM, SVDConv2dC, SVDConv2dM)

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64, dilation=1, norm_layer=None,
                 stage=1, id=0, conv=TTConv2dR, hp_dict=None, dense_dict=None):
        super().__init__()
        if norm_layer is None:
            norm_layer = nn.BatchNorm2d
        width = int(planes * (base_width / 64.)) * groups
        # both self.conv2 and self.downsample downsample the input when stride != 1
        w_name, listed, dense_w = _named(hp_dict, dense_dict, stage, id, 'conv1')
        self.conv1 = tt_conv1x1(inplanes, width, conv=conv, hp_dict=hp_dict, name=w_name, dense_w=dense_w) \
            if listed else conv1x1(inplanes, width)
        self.bn1 = norm_layer(width)
        w_name, listed, dense_w = _named(hp_dict, dense_dict, stage, id, 'conv2')
        self.conv2 = tt_conv3x3(width, width, stride, groups, dilation, conv=conv, hp_dict=hp_dict, name=w_name,
                                dense_w=dense_w) if listed else conv3x3(width, width, stride, groups, dilation)
        self.bn2 = norm_layer(width)
        w_name, listed, dense_w = _named(hp_dict, dense_dict, stage, id, 'conv3')
        self.conv3 = tt_conv1x1(width, planes * self.expansion, conv=conv, hp_dict=hp_dict, name=w_name, dense_w=dense_w) \
            if listed else conv1x1(width, planes * self.expansion)
        self.bn3 = norm_layer(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        out = self._bn(self.bn1, self.conv1(x))
        out = self._bn(self.bn2, self.conv2(out))
        return self._bn(self.bn3, self.conv3(out), self._identity(x))

    def forward_flops(self, x, name):
        base_flops = compr_flops = 0
        out = x
        for which, bn in (('conv1', self.bn1), ('conv2', self.bn2), ('conv3', self.bn3)):
            print('>{}:'.format(name + which))
            out, flops1, flops2 = _conv_flops(getattr(self, which), out, self._flops_layers)
            base_flops += flops1
            compr_flops += flops2
            out = self._bn(bn, out, self._identity(x)) if which == 'conv3' else self._bn(bn, out)
        return out, base_flops, compr_flops


class TTResNet(_Routed):
    def __init__(self, block, layers, num_classes=1000, zero_init_residual=False, groups=1, width_per_group=64,
                 replace_stride_with_dilation=None, norm_layer=None, conv=TTConv2dR, hp_dict=None, dense_dict=None):
        super().__init__()
        if norm_layer is None:
            norm_layer = nn.BatchNorm2d
        self._norm_layer = norm_layer
        self.inplanes = 64
        self.dilation = 1
        if replace_stride_with_dilation is None:
            # each element says whether the 2x2 stride is replaced with a dilated convolution
            replace_stride_with_dilation = [False, False, False]
        if len(replace_stride_with_dilation) != 3:
            raise ValueError("replace_stride_with_dilation should be None "
                             "or a 3-element tuple, got {}".format(replace_stride_with_dilation))
        self.groups = groups
        self.base_width = width_per_group
        self.conv1 = nn.Conv2d(3, self.inplanes, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = norm_layer(self.inplanes)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        kw = dict(conv=conv, hp_dict=hp_dict, dense_dict=dense_dict)
        self.layer1 = self._make_layer(block, 64, layers[0], stage=1, **kw)
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2, dilate=replace_stride_with_dilation[0], stage=2, **kw)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2, dilate=replace_stride_with_dilation[1], stage=3, **kw)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2, dilate=replace_stride_with_dilation[2], stage=4, **kw)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * block.expansion, num_classes)

        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        # zero-initialise the last BatchNorm of each residual branch, so that a block starts as the identity
        # (https://arxiv.org/abs/1706.02677)
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, TTBottleneck):
                    nn.init.constant_(m.bn3.weight, 0)
                elif isinstance(m, TTBasicBlock):
                    nn.init.constant_(m.bn2.weight, 0)

    def _make_layer(self, block, planes, blocks, stride=1, dilate=False, stage=1, conv=TTConv2dR, hp_dict=None,
                    dense_dict=None):
        norm_layer = self._norm_layer
        downsample = None
        previous_dilation = self.dilation
        if dilate:
            self.dilation *= stride
            stride = 1
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(conv1x1(self.inplanes, planes * block.expansion, stride),
                                       norm_layer(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample, self.groups, self.base_width, previous_dilation,
                        norm_layer, stage=stage, id=0, conv=conv, hp_dict=hp_dict, dense_dict=dense_dict)]
        self.inplanes = planes * block.expansion
        for id in range(1, blocks):
            layers.append(block(self.inplanes, planes, groups=self.groups, base_width=self.base_width,
                                dilation=self.dilation, norm_layer=norm_layer, stage=stage, id=id, conv=conv,
                                hp_dict=hp_dict, dense_dict=dense_dict))
        return nn.Sequential(*layers)

    def set_route(self, route):
        """Forces one route (None, "launch", "composed") on every BatchNorm tail; returns self."""
        for m in self.modules():
            if isinstance(m, _Routed):
                m.route = route
        return self

    def _stem(self, x):
        return self.maxpool(self._bn(self.bn1, self.conv1(x)))

    def _head(self, x):
        return self.fc(torch.flatten(self.avgpool(x), 1))

    def forward(self, x):
        x = self._stem(x)
        x = self.layer1(x)
        x = self.layer2(x)
        x = self.layer3(x)
        x = self.layer4(x)
        return self._head(x)

    def forward_flops(self, x):
        x = self._stem(x)
        base_flops = compr_flops = 0
        for s, layer in enumerate((self.layer1, self.layer2, self.layer3, self.layer4), 1):
            for i, block in enumerate(layer):
                x, flops1, flops2 = block.forward_flops(x, 'layer{}.{}.'.format(s, i))
                base_flops += flops1
                compr_flops += flops2
        return self._head(x), base_flops, compr_flops


def _tt_resnet(block, layers, conv, hp_dict, dense_dict=None, **kwargs):
    model = TTResNet(block, layers, conv=conv, hp_dict=hp_dict, dense_dict=dense_dict, **kwargs)
    if dense_dict is not None:                  # the dense parts take the dense model's values
        tt_dict = model.state_dict()
        for key in tt_dict:
            if key in dense_dict:
                tt_dict[key] = dense_dict[key]
        model.load_state_dict(tt_dict)
    return model


def _factory(name, conv, block, layers):
    def create(hp_dict, decompose=False, pretrained=False, path=None, dense_dict=None, **kwargs):
        # the reference downloads timm's dense model when decompose and pretrained are both set; here `path` is read
        return create_model(name, partial(_tt_resnet, block, layers, conv=conv, **kwargs), hp_dict, decompose, pretrained,
                            path, dense_dict)
    create.__name__ = create.__qualname__ = name
    create.__doc__ = (f"resnet_inet_tt.py: {name}(hp_dict, decompose=False, pretrained=False, path=None, dense_dict=None, "
                      "**kwargs).  decompose=True factorises the dense state dict given as dense_dict= (or saved at the "
                      "local `path`); pretrained=True without decompose loads a compressed state dict from the local `path`.")
    return create


_ARCH = {"resnet18": (TTBasicBlock, [2, 2, 2, 2]), "resnet34": (TTBasicBlock, [3, 4, 6, 3]),
         "resnet50": (TTBottleneck, [3, 4, 6, 3])}
_CONV = {"ttr": TTConv2dR, "ttm": TTConv2dM, "tkc": TKConv2dC, "tkm": TKConv2dM, "tkr": TKConv2dR}
# the eleven the reference defines
FACTORIES = ("ttr_resnet18", "ttm_resnet18", "tkc_resnet18", "tkm_resnet18", "ttr_resnet34", "ttr_resnet50", "tkr_resnet18",
             "tkr_resnet34", "tkr_resnet50", "tkm_resnet50", "tkc_resnet50")
for _name in FACTORIES:
    _kind, _arch = _name.split("_")
    globals()[_name] = _factory(_name, _CONV[_kind], *_ARCH[_arch])
del _name, _kind, _arch

__all__ = ["conv3x3", "conv1x1", "tt_conv3x3", "tt_conv1x1", "TTBasicBlock", "TTBottleneck", "TTResNet", "FACTORIES"] \
    + list(FACTORIES)
