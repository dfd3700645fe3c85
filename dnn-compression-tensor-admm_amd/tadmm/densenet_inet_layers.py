"""The ImageNet DenseNets of the reference's main path (densenet_inet_tt.py: TenDenseLayer, TenDenseBlock,
TenDenseTransition, TenDenseNet with its stem options and `memory_efficient`, and the `tkc_densenet121` / `201` / `264`
factories), without timm.  State-dict keys are timm's DenseNet (features.conv0, features.norm0,
features.denseblock{S}.denselayer{I}.norm1 / conv1 / norm2 / conv2, features.transition{S}.norm / conv, features.norm5,
classifier) with the factorised layers' own keys in place of the replaced weights; the initialisation is the reference's.

`norm_layer` builds `BatchNormAct2d`, the stand-in for timm's layer of that name: an nn.BatchNorm2d (the same five
state-dict entries) followed by ReLU.  Called on the features of a dense block (a `functional.DenseFeatures` or a list
of tensors) it goes through `functional.dense_batch_norm_act` (csrc/densebn.hip): every channel is read from the feature
tensor that owns it and the batch statistics are those the holder computed once per tensor, so norm1 of every layer, the
transition's norm and norm5 never see a concatenation on the launch route.  Called on one tensor (norm0, norm2) it goes
through `functional.batch_norm_act` (csrc/bnact.hip).  As in the reference, conv1 and the transition's conv are
SVDConv2dC when their weight name is in `hp_dict.ranks` whatever `conv` is, and conv2 is `conv` (TKConv2dC in the
factories); the others are nn.Conv2d.  `memory_efficient=True` keeps the reference's checkpointed bottleneck, on the
composed route (torch.cat inside the checkpoint).  Nothing is ever downloaded: where the reference fetches timm's
pretrained dense model (`decompose=True, pretrained=True`), the dense state dict comes from `dense_dict=` or a local file.
No rank table ships for densenet264; its factory takes the caller's `hp_dict`."""
from collections import OrderedDict
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint as cp

from . import functional as HF
from .functional import DenseFeatures
from .svd_layers import SVDConv2dC
from .tk_layers import TKConv2dC
from ._layer_common import create_model


class BatchNormAct2d(nn.BatchNorm2d):
    """BatchNorm2d + ReLU with the state-dict entries of nn.BatchNorm2d.  The input is one (N, C, H, W) tensor or the
    feature tensors of a dense block, whose channels add up to `num_features`."""
    route = None                                # None: the measured rule; "launch" / "composed" force a route

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, apply_act=True):
        super().__init__(num_features, eps=eps, momentum=momentum, affine=affine, track_running_stats=track_running_stats)
        self.apply_act = apply_act

    def forward(self, x):
        if isinstance(x, torch.Tensor):
            return HF.batch_norm_act_module(self, x, relu=self.apply_act, route=self.route)
        return HF.dense_batch_norm_act_module(self, x, route=self.route, relu=self.apply_act)


def _named_conv(listed_cls, hp_dict, dense_dict, w_name, cin, cout, kernel_size, padding=0):
    if hp_dict is not None and w_name in hp_dict.ranks:
        return listed_cls(cin, cout, kernel_size=kernel_size, stride=1, padding=padding, bias=False, hp_dict=hp_dict,
                          name=w_name, dense_w=None if not dense_dict else dense_dict[w_name])
    return nn.Conv2d(cin, cout, kernel_size=kernel_size, stride=1, padding=padding, bias=False)


class TenDenseLayer(nn.Module):
    def __init__(self, num_input_features, growth_rate, bn_size, norm_layer=BatchNormAct2d, drop_rate=0.,
                 memory_efficient=False, conv=TKConv2dC, stage=None, id=None, hp_dict=None, dense_dict=None):
        super().__init__()
        pre = 'features.denseblock' + str(stage) + '.denselayer' + str(id)
        self.add_module('norm1', norm_layer(num_input_features))
        self.add_module('conv1', _named_conv(SVDConv2dC, hp_dict, dense_dict, pre + '.conv1.weight', num_input_features,
                                             bn_size * growth_rate, 1))
        self.add_module('norm2', norm_layer(bn_size * growth_rate))
        self.add_module('conv2', _named_conv(conv, hp_dict, dense_dict, pre + '.conv2.weight', bn_size * growth_rate,
                                             growth_rate, 3, 1))
        self.drop_rate = float(drop_rate)
        self.memory_efficient = memory_efficient

    def bottleneck_fn(self, xs):
        """conv1(norm1(features)): `xs` is a DenseFeatures, or a list of tensors (concatenated by the composed route)."""
        return self.conv1(self.norm1(xs))

    def any_requires_grad(self, x):
        return any(t.requires_grad for t in x)

    def call_checkpoint_bottleneck(self, x):
        def closure(*xs):
            return self.conv1(self.norm1(torch.cat(xs, 1)))

        return cp.checkpoint(closure, *x, use_reentrant=True)

    def forward(self, x):
        prev_features = DenseFeatures(x) if isinstance(x, torch.Tensor) else x
        if self.memory_efficient and self.any_requires_grad(prev_features):
            bottleneck_output = self.call_checkpoint_bottleneck(list(prev_features))
        else:
            bottleneck_output = self.bottleneck_fn(prev_features)
        new_features = self.conv2(self.norm2(bottleneck_output))
        if self.drop_rate > 0:
            new_features = F.dropout(new_features, p=self.drop_rate, training=self.training)
        return new_features


class TenDenseBlock(nn.ModuleDict):
    _version = 2

    def __init__(self, num_layers, num_input_features, bn_size, growth_rate, norm_layer=BatchNormAct2d, drop_rate=0.,
                 memory_efficient=False, conv=TKConv2dC, stage=None, hp_dict=None, dense_dict=None):
        super().__init__()
        for i in range(num_layers):
            layer = TenDenseLayer(num_input_features + i * growth_rate, growth_rate=growth_rate, bn_size=bn_size,
                                  norm_layer=norm_layer, drop_rate=drop_rate, memory_efficient=memory_efficient,
                                  conv=conv, stage=stage, id=i + 1, hp_dict=hp_dict, dense_dict=dense_dict)
            self.add_module('denselayer%d' % (i + 1), layer)

    def set_route(self, route):
        return set_route(self, route)

    def forward(self, init_features):
        """The block's features as one `DenseFeatures` (the input first); `.cat()` is the reference's output."""
        features = DenseFeatures(init_features.contiguous())
        for name, layer in self.items():
            features.append(layer(features).contiguous())    # NCHW contiguous: every later layer reads it in place
        return features


class TenDenseTransition(nn.Sequential):
    """norm, conv, pool; the norm takes the dense block's `DenseFeatures` as it is."""

    def __init__(self, num_input_features, num_output_features, norm_layer=BatchNormAct2d, aa_layer=None, stage=None,
                 hp_dict=None, dense_dict=None):
        super().__init__()
        self.add_module('norm', norm_layer(num_input_features))
        self.add_module('conv', _named_conv(SVDConv2dC, hp_dict, dense_dict,
                                            'features.transition' + str(stage) + '.conv.weight', num_input_features,
                                            num_output_features, 1))
        if aa_layer is not None:
            self.add_module('pool', aa_layer(num_output_features, stride=2))
        else:
            self.add_module('pool', nn.AvgPool2d(kernel_size=2, stride=2))

    def set_route(self, route):
        return set_route(self, route)


class _GlobalPool(nn.Module):
    """timm's SelectAdaptivePool2d(pool_type, flatten=True) for 'avg', 'max' and '' (no pooling, no flatten)."""

    def __init__(self, pool_type='avg'):
        super().__init__()
        if pool_type not in ('avg', 'max', ''):
            raise ValueError(f"global_pool is 'avg', 'max' or '' (got {pool_type!r})")
        self.pool_type = pool_type

    def forward(self, x):
        if self.pool_type == '':
            return x
        pooled = F.adaptive_avg_pool2d(x, 1) if self.pool_type == 'avg' else F.adaptive_max_pool2d(x, 1)
        return pooled.flatten(1)


def _create_classifier(num_features, num_classes, pool_type='avg'):
    fc = nn.Linear(num_features, num_classes, bias=True) if num_classes > 0 else nn.Identity()
    return _GlobalPool(pool_type), fc


class TenDenseNet(nn.Module):
    r"""Densenet-BC model class, based on
    `"Densely Connected Convolutional Networks" <https://arxiv.org/pdf/1608.06993.pdf>`_

    Args:
        growth_rate (int) - how many filters to add each layer (`k` in paper)
        block_config (list of ints) - how many layers in each pooling block
        bn_size (int) - multiplicative factor for number of bottle neck layers
          (i.e. bn_size * k features in the bottleneck layer)
        drop_rate (float) - dropout rate after each dense layer
        num_classes (int) - number of classification classes
        memory_efficient (bool) - If True, uses checkpointing (and the composed route in the bottleneck)
    """

    def __init__(self, growth_rate=32, block_config=(6, 12, 24, 16), bn_size=4, stem_type='', num_classes=1000, in_chans=3,
                 global_pool='avg', norm_layer=BatchNormAct2d, aa_layer=None, drop_rate=0, memory_efficient=False,
                 aa_stem_only=True, conv=TKConv2dC, hp_dict=None, dense_dict=None):
        self.num_classes = num_classes
        self.drop_rate = drop_rate
        super().__init__()

        # Stem
        deep_stem = 'deep' in stem_type  # 3x3 deep stem
        num_init_features = growth_rate * 2
        if aa_layer is None:
            stem_pool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        else:
            stem_pool = nn.Sequential(*[
                nn.MaxPool2d(kernel_size=3, stride=1, padding=1),
                aa_layer(channels=num_init_features, stride=2)])
        if deep_stem:
            stem_chs_1 = stem_chs_2 = growth_rate
            if 'tiered' in stem_type:
                stem_chs_1 = 3 * (growth_rate // 4)
                stem_chs_2 = num_init_features if 'narrow' in stem_type else 6 * (growth_rate // 4)
            self.features = nn.Sequential(OrderedDict([
                ('conv0', nn.Conv2d(in_chans, stem_chs_1, 3, stride=2, padding=1, bias=False)),
                ('norm0', norm_layer(stem_chs_1)),
                ('conv1', nn.Conv2d(stem_chs_1, stem_chs_2, 3, stride=1, padding=1, bias=False)),
                ('norm1', norm_layer(stem_chs_2)),
                ('conv2', nn.Conv2d(stem_chs_2, num_init_features, 3, stride=1, padding=1, bias=False)),
                ('norm2', norm_layer(num_init_features)),
                ('pool0', stem_pool),
            ]))
        else:
            self.features = nn.Sequential(OrderedDict([
                ('conv0', nn.Conv2d(in_chans, num_init_features, kernel_size=7, stride=2, padding=3, bias=False)),
                ('norm0', norm_layer(num_init_features)),
                ('pool0', stem_pool),
            ]))
        self.feature_info = [
            dict(num_chs=num_init_features, reduction=2, module=f'features.norm{2 if deep_stem else 0}')]
        current_stride = 4

        # DenseBlocks
        num_features = num_init_features
        for i, num_layers in enumerate(block_config):
            block = TenDenseBlock(num_layers=num_layers, num_input_features=num_features, bn_size=bn_size,
                                  growth_rate=growth_rate, norm_layer=norm_layer, drop_rate=drop_rate,
                                  memory_efficient=memory_efficient, conv=conv, stage=i + 1, hp_dict=hp_dict,
                                  dense_dict=dense_dict)
            module_name = f'denseblock{(i + 1)}'
            self.features.add_module(module_name, block)
            num_features = num_features + num_layers * growth_rate
            transition_aa_layer = None if aa_stem_only else aa_layer
            if i != len(block_config) - 1:
                self.feature_info += [
                    dict(num_chs=num_features, reduction=current_stride, module='features.' + module_name)]
                current_stride *= 2
                trans = TenDenseTransition(num_input_features=num_features, num_output_features=num_features // 2,
                                           norm_layer=norm_layer, aa_layer=transition_aa_layer, stage=i + 1,
                                           hp_dict=hp_dict, dense_dict=dense_dict)
                self.features.add_module(f'transition{i + 1}', trans)
                num_features = num_features // 2

        # Final batch norm: takes the last block's DenseFeatures
        self.features.add_module('norm5', norm_layer(num_features))

        self.feature_info += [dict(num_chs=num_features, reduction=current_stride, module='features.norm5')]
        self.num_features = num_features

        # Linear layer
        self.global_pool, self.classifier = _create_classifier(self.num_features, self.num_classes, pool_type=global_pool)

        # Official init from torch repo.
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Linear):
                nn.init.constant_(m.bias, 0)

    def set_route(self, route):
        """Forces one route (None, "launch", "composed") on every BatchNormAct2d; returns self."""
        return set_route(self, route)

    def get_classifier(self):
        return self.classifier

    def reset_classifier(self, num_classes, global_pool='avg'):
        self.num_classes = num_classes
        self.global_pool, self.classifier = _create_classifier(self.num_features, self.num_classes, pool_type=global_pool)

    def forward_features(self, x):
        return self.features(x)

    def forward(self, x):
        x = self.forward_features(x)
        x = self.global_pool(x)
        x = self.classifier(x)
        return x


def set_route(module, route):
    """Forces one route (None, "launch", "composed") on every BatchNormAct2d inside `module`; returns the module."""
    if route not in (None, "launch", "composed"):
        raise ValueError(f"route is None, 'launch' or 'composed' (got {route!r})")
    for m in module.modules():
        if isinstance(m, BatchNormAct2d):
            m.route = route
    return module


def _ten_densenet(growth_rate=32, block_config=(6, 12, 24, 16), num_classes=1000, conv=TKConv2dC, hp_dict=None,
                  dense_dict=None, **kwargs):
    if 'num_classes' in kwargs:
        num_classes = kwargs.pop('num_classes')
    model = TenDenseNet(growth_rate, block_config, num_classes=num_classes, conv=conv, hp_dict=hp_dict,
                        dense_dict=dense_dict, **kwargs)
    if dense_dict is not None:                  # the dense parts take the dense model's values
        ten_dict = model.state_dict()
        for key in ten_dict:
            if key in dense_dict:
                ten_dict[key] = dense_dict[key]
        model.load_state_dict(ten_dict)
    return model


def _factory(name, growth_rate, block_config):
    def create(hp_dict, decompose=False, pretrained=False, path=None, dense_dict=None, **kwargs):
        build = partial(_ten_densenet, growth_rate=growth_rate, block_config=block_config, conv=TKConv2dC, **kwargs)
        return create_model(name, build, hp_dict, decompose, pretrained, path, dense_dict)
    create.__name__ = create.__qualname__ = name
    create.__doc__ = (f"densenet_inet_tt.py: {name}(hp_dict, decompose=False, pretrained=False, path=None, **kwargs): growth "
                      f"{growth_rate}, blocks {block_config}.  decompose=True factorises the dense state dict given as "
                      "dense_dict= (or saved at the local `path`); pretrained=True alone loads a compressed state dict from "
                      "the local `path`.")
    return create


tkc_densenet121 = _factory("tkc_densenet121", 32, (6, 12, 24, 16))
tkc_densenet201 = _factory("tkc_densenet201", 32, (6, 12, 48, 32))
tkc_densenet264 = _factory("tkc_densenet264", 48, (6, 12, 64, 48))
FACTORIES = ("tkc_densenet121", "tkc_densenet201", "tkc_densenet264")

__all__ = ["BatchNormAct2d", "TenDenseLayer", "TenDenseBlock", "TenDenseTransition", "TenDenseNet", "set_route",
           "FACTORIES"] + list(FACTORIES)
