"""What the TT, Tucker and SVD layer files share: the bias constructor, the dense convolution of the R variants and the
eligibility test of the fused linear chain -- and what the model files share: the local state-dict loader and the body
of their factories."""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.modules.utils import _pair, _reverse_repeat_tuple

from . import functional as HF
from . import ops


def make_bias(layer: nn.Module, n: int, bias: bool, dense_b) -> None:
    """Registers `layer.bias`: n zeros, re-pointed at `dense_b` where given, or None.
    Deliberate deviation: the reference allocates the bias with `torch.Tensor(n)` (TTLinear.py:53, TTConv.py:254) and
    the M variants (and every layer built from `dense_w` without `dense_b`) never initialise it -- it holds whatever the
    allocator hands out, NaNs included.  Zeros are one of the values that memory can hold; `reset_parameters` of the R
    variants overwrites them as the reference does."""
    if bias:
        layer.bias = nn.Parameter(torch.zeros(n))
        if dense_b is not None:
            layer.bias.data = dense_b
    else:
        layer.register_parameter('bias', None)


class DenseConvMixin:
    """The R variants: conv2d with the dense kernel rebuilt from the factors, any `padding_mode` and `groups` of nn.Conv2d."""

    def _init_dense_conv(self, in_channels, out_channels, groups, padding_mode):
        """The argument checks of the reference's R layers; call once `self.padding` is set."""
        if in_channels % groups != 0:
            raise ValueError('in_channels must be divisible by groups')
        if out_channels % groups != 0:
            raise ValueError('out_channels must be divisible by groups')
        valid_padding_modes = {'zeros', 'reflect', 'replicate', 'circular'}
        if padding_mode not in valid_padding_modes:
            raise ValueError("padding_mode must be one of {}, but got padding_mode='{}'".format(
                valid_padding_modes, padding_mode))
        self._reversed_padding_repeated_twice = _reverse_repeat_tuple(self.padding, 2)

    def _conv_forward(self, x, weight):
        if self.padding_mode != 'zeros':
            return F.conv2d(F.pad(x, self._reversed_padding_repeated_twice, mode=self.padding_mode), weight, self.bias,
                            self.stride, _pair(0), self.dilation, self.groups)
        return F.conv2d(x, weight, self.bias, self.stride, self.padding, self.dilation, self.groups)

    def forward(self, x):
        return self._conv_forward(x, self._recover_weight())


def _local_state_dict(path, what):
    if path is None:
        raise ValueError(f"{what}: give the dense state dict as dense_dict= or a local file as path=; nothing is downloaded")
    if str(path).startswith('http'):
        raise ValueError(f"{what}: path is a URL ({path}); nothing is downloaded -- fetch the file and pass its local path")
    return torch.load(path, map_location='cpu')


def create_model(name, build, hp_dict, decompose, pretrained, path, dense_dict, load_with_decompose=False):
    """The body of every model factory `name(hp_dict, decompose, pretrained, path, dense_dict, **kwargs)`.
    `build(hp_dict=, dense_dict=)` makes the model: with `decompose` it factorises the dense state dict given as
    `dense_dict` (or saved at the local `path`), without it `dense_dict` is ignored.  `pretrained` then loads a
    compressed state dict from the local `path` -- only without `decompose`, unless `load_with_decompose` says that
    this factory of the reference loads it either way."""
    if decompose:
        if dense_dict is None:
            dense_dict = _local_state_dict(path, name + "(decompose=True)")
    else:
        dense_dict = None
    model = build(hp_dict=hp_dict, dense_dict=dense_dict)
    if pretrained and (load_with_decompose or not decompose):
        model.load_state_dict(_local_state_dict(path, name + "(pretrained=True)"))
    return model


def fused_linear_ok(x, bias, params, rank: int, in_features: int, out_features: int) -> bool:
    """True when a linear layer through middle rank `rank` is one launch of the fused chain (`functional.linear_chain`):
    a dtype the chain takes on behalf of these parameters (float16 is inference only), a rank that fits the LDS, and
    rows of whole 16-byte units.  The backward runs the same kernels with the gradient as X (row length out_features):
    a head whose width is not 16-byte aligned (10 classes) is eligible only while nothing wants a gradient."""
    align = 8 if x.dtype in ops.HALF_DTYPES else 4
    if not (HF.chain_dtype_ok(x, bias, *params) and HF.fused_rank_ok(rank) and in_features % align == 0):
        return False
    return out_features % align == 0 or not HF._needs_grad(x, bias, *params)
