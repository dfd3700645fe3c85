"""The CIFAR DenseNet of the reference's main path (densenet_cifar_tt.py: TenBasicBlock, TenBottleneckBlock,
TenTransitionBlock, TenDenseBlock, TenDenseNet and the `tkr_densenet40` factory), without timm.  State-dict keys
(conv1, block{S}.layer.{I}.bn1 / conv1 / bn2 / conv2, trans{S}.bn1 / conv1, bn1, fc), initialisation and constructor
arguments are the reference's, so a `densenet40` checkpoint decomposes and a compressed one loads as they do there; the
BatchNorm modules stay nn.BatchNorm2d.

Where the reference's layers hand `torch.cat([x, out], 1)` to the next layer, a block here passes one
`functional.DenseFeatures` from layer to layer: every pre-activation relu(bn1(cat(features))) goes through
`functional.dense_batch_norm_act` (csrc/densebn.hip), which reads each channel from the feature tensor that owns it
and takes the batch statistics the holder computed once per tensor.  The transition and the network's final bn1 consume
the list directly, so on the launch route no concatenation is ever formed.  The bottleneck's relu(bn2(.)) has one input
tensor and goes through `functional.batch_norm_act` (csrc/bnact.hip).  Dropout and `avg_pool2d` stay with torch.  `conv`
is one of TKConv2dR / TKConv2dM / TKConv2dC / TTConv2dM / TTConv2dR and builds the convolutions whose weight name is in
`hp_dict.ranks`; the others are nn.Conv2d.  Nothing is ever downloaded: a dense state dict comes from `dense_dict=` or
a local file.

Every block and the network also take a plain (N, C, H, W) tensor where they take a `DenseFeatures`; a block returns
the holder (`.cat()` gives the reference's tensor)."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as HF
from .functional import DenseFeatures
from .tk_layers import TKConv2dC, TKConv2dM, TKConv2dR
from .tt_layers import TTConv2dM, TTConv2dR
from ._layer_common import _local_state_dict


def _conv(conv, hp_dict, dense_dict, w_name, in_planes, planes, kernel_size, padding):
    if hp_dict is not None and w_name in hp_dict.ranks:
        return conv(in_planes, planes, kernel_size=kernel_size, stride=1, padding=padding, bias=False, hp_dict=hp_dict,
                    name=w_name, dense_w=None if dense_dict is None else dense_dict[w_name])
    return nn.Conv2d(in_planes, planes, kernel_size=kernel_size, stride=1, padding=padding, bias=False)


def _grown(layer, x):
    """The holder with the layer's new features appended; a plain tensor starts one.  A feature tensor is stored NCHW
    contiguous (a factorised convolution may hand out another layout): the launch reads it in place in every later layer."""
    feats = x if isinstance(x, DenseFeatures) else DenseFeatures(x.contiguous())
    return feats.append(layer.new_features(feats).contiguous())


class _Routed(nn.Module):
    route = None                                # None: the measured rule; "launch" / "composed" force a route

    def set_route(self, route):
        """Forces one route (None, "launch", "composed") on every BatchNorm of the module; returns self."""
        for m in self.modules():
            if isinstance(m, _Routed):
                m.route = route
        return self

    def _drop(self, out):
        if self.droprate > 0:
            out = F.dropout(out, p=self.droprate, training=self.training)
        return out


class TenBasicBlock(_Routed):
    def __init__(self, in_planes, out_planes, dropRate=0.0, conv=TKConv2dR, stage=None, id=None, hp_dict=None,
                 dense_dict=None):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(in_planes)
        self.relu = nn.ReLU(inplace=True)
        pre = 'block' + str(stage) + '.layer.' + str(id)
        self.conv1 = _conv(conv, hp_dict, dense_dict, pre + '.conv1.weight', in_planes, out_planes, 3, 1)
        self.droprate = dropRate

    def new_features(self, feats):
        """The layer's growth_rate new channels from the features so far."""
        return self._drop(self.conv1(HF.dense_batch_norm_act_module(self.bn1, feats, route=self.route)))

    def forward(self, x):
        return _grown(self, x)


class TenBottleneckBlock(_Routed):
    def __init__(self, in_planes, out_planes, dropRate=0.0, conv=TKConv2dR, stage=None, id=None, hp_dict=None,
                 dense_dict=None):
        super().__init__()
        inter_planes = out_planes * 4
        self.bn1 = nn.BatchNorm2d(in_planes)
        self.relu = nn.ReLU(inplace=True)
        pre = 'block' + str(stage) + '.layer.' + str(id)
        self.conv1 = _conv(conv, hp_dict, dense_dict, pre + '.conv1.weight', in_planes, inter_planes, 1, 0)
        self.bn2 = nn.BatchNorm2d(inter_planes)
        self.conv2 = _conv(conv, hp_dict, dense_dict, pre + '.conv2.weight', inter_planes, out_planes, 3, 1)
        self.droprate = dropRate

    def new_features(self, feats):
        out = self._drop(self.conv1(HF.dense_batch_norm_act_module(self.bn1, feats, route=self.route)))
        return self._drop(self.conv2(HF.batch_norm_act_module(self.bn2, out, route=self.route)))

    def forward(self, x):
        return _grown(self, x)


class TenTransitionBlock(_Routed):
    def __init__(self, in_planes, out_planes, dropRate=0.0, conv=TKConv2dR, stage=None, hp_dict=None, dense_dict=None):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(in_planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv1 = _conv(conv, hp_dict, dense_dict, 'trans' + str(stage) + '.conv1.weight', in_planes, out_planes, 1, 0)
        self.droprate = dropRate

    def forward(self, x):
        out = self._drop(self.conv1(HF.dense_batch_norm_act_module(self.bn1, x, route=self.route)))
        return F.avg_pool2d(out, 2)


class TenDenseBlock(_Routed):
    def __init__(self, nb_layers, in_planes, growth_rate, block, dropRate=0.0, conv=TKConv2dR, stage=None, hp_dict=None,
                 dense_dict=None):
        super().__init__()
        self.layer = self._make_layer(block, in_planes, growth_rate, nb_layers, dropRate, conv, stage, hp_dict,
                                      dense_dict)

    def _make_layer(self, block, in_planes, growth_rate, nb_layers, dropRate, conv, stage, hp_dict, dense_dict):
        layers = []
        for i in range(nb_layers):
            layers.append(block(in_planes + i * growth_rate, growth_rate, dropRate, conv, stage, i, hp_dict, dense_dict))
        return nn.Sequential(*layers)

    def forward(self, x):
        """The block's features as one `DenseFeatures` (the input first); `.cat()` is the reference's output."""
        feats = DenseFeatures(x.contiguous()) if isinstance(x, torch.Tensor) else x
        for layer in self.layer:
            feats = layer(feats)
        return feats


class TenDenseNet(_Routed):
    def __init__(self, depth, num_classes=10, growth_rate=12, reduction=0.5, bottleneck=True, dropRate=0.0,
                 conv=TKConv2dR, hp_dict=None, dense_dict=None):
        super().__init__()
        in_planes = 2 * growth_rate
        n = (depth - 4) / 3
        if bottleneck:
            n = n / 2
            block = TenBottleneckBlock
        else:
            block = TenBasicBlock
        n = int(n)
        # 1st conv before any dense block
        self.conv1 = nn.Conv2d(3, in_planes, kernel_size=3, stride=1, padding=1, bias=False)
        # 1st block
        self.block1 = TenDenseBlock(n, in_planes, growth_rate, block, dropRate, conv, 1, hp_dict, dense_dict)
        in_planes = int(in_planes + n * growth_rate)
        self.trans1 = TenTransitionBlock(in_planes, int(math.floor(in_planes * reduction)), dropRate, conv, 1, hp_dict,
                                         dense_dict)
        in_planes = int(math.floor(in_planes * reduction))
        # 2nd block
        self.block2 = TenDenseBlock(n, in_planes, growth_rate, block, dropRate, conv, 2, hp_dict, dense_dict)
        in_planes = int(in_planes + n * growth_rate)
        self.trans2 = TenTransitionBlock(in_planes, int(math.floor(in_planes * reduction)), dropRate, conv, 2, hp_dict,
                                         dense_dict)
        in_planes = int(math.floor(in_planes * reduction))
        # 3rd block
        self.block3 = TenDenseBlock(n, in_planes, growth_rate, block, dropRate, conv, 3, hp_dict, dense_dict)
        in_planes = int(in_planes + n * growth_rate)
        # global average pooling and classifier
        self.bn1 = nn.BatchNorm2d(in_planes)
        self.relu = nn.ReLU(inplace=True)
        self.fc = nn.Linear(in_planes, num_classes)
        self.in_planes = in_planes

        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()
            elif isinstance(m, nn.Linear):
                m.bias.data.zero_()

    def forward(self, x):
        out = self.conv1(x)
        out = self.trans1(self.block1(out))
        out = self.trans2(self.block2(out))
        out = self.block3(out)
        out = HF.dense_batch_norm_act_module(self.bn1, out, route=self.route)
        out = F.avg_pool2d(out, 8)
        out = out.view(-1, self.in_planes)
        return self.fc(out)


def _ten_densenet(num_layers, grow_rate=16, num_classes=10, reduction=0.5, bottleneck=False, conv=TKConv2dR,
                  hp_dict=None, dense_dict=None, **kwargs):
    if 'num_classes' in kwargs:
        num_classes = kwargs.pop('num_classes')
    model = TenDenseNet(num_layers, num_classes, grow_rate, reduction, bottleneck, conv=conv, hp_dict=hp_dict,
                        dense_dict=dense_dict, **kwargs)
    if dense_dict is not None:                  # the dense parts take the dense model's values
        ten_dict = model.state_dict()
        for key in ten_dict:
            if key in dense_dict:
                ten_dict[key] = dense_dict[key]
        model.load_state_dict(ten_dict)
    return model


def tkr_densenet40(hp_dict, decompose=False, pretrained=False, path=None, dense_dict=None, **kwargs):
    """densenet_cifar_tt.py: tkr_densenet40(hp_dict, decompose=False, pretrained=False, path=None, **kwargs): depth 40,
    growth 16, basic blocks, TKConv2dR.  decompose=True factorises the dense state dict given as dense_dict= (or saved
    at the local `path`); pretrained=True loads a compressed state dict from the local `path`."""
    if decompose:
        if dense_dict is None:
            dense_dict = _local_state_dict(path, "tkr_densenet40(decompose=True)")
    else:
        dense_dict = None
    model = _ten_densenet(40, bottleneck=False, conv=TKConv2dR, hp_dict=hp_dict, dense_dict=dense_dict, **kwargs)
    if pretrained:
        model.load_state_dict(_local_state_dict(path, "tkr_densenet40(pretrained=True)"))
    return model


FACTORIES = ("tkr_densenet40",)

__all__ = ["TenBasicBlock", "TenBottleneckBlock", "TenTransitionBlock", "TenDenseBlock", "TenDenseNet", "FACTORIES",
           "tkr_densenet40"]
