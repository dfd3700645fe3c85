"""Rank-r SVD-factorised 1x1 convolutions with the reference's constructor signatures and state_dict keys (SVDConv.py).

  SVDConv2dR : rebuild the dense 1x1 kernel + conv2d         (left_factor, right_factor, bias)
  SVDConv2dC : 1x1 conv (C -> r) -> 1x1 conv (r -> O)        (bias, left_kernel, right_kernel)
  SVDConv2dM : per-pixel linear (C -> r) -> linear (r -> O)  (bias, left_factor, right_factor)

`dense_w` is decomposed by a one-layer device SVD plan (`ops.ProjectionPlan`, KIND_SVD, the projection the ADMM phase
runs for these layers): core 0 of the plan is U (O x r), core 1 carries the singular values, diag(s) V^T (r x I).  The
reference's CPU LAPACK SVD gives the same factors up to the sign of each singular pair.

C and M run on the chain kernels, on the NCHW tensors in place, for float32 / bfloat16 inputs and, in inference, float16
ones (what `evaluate()` under autocast sends): the 16-bit types with a rank up to 256 as one launch of the fused chain
(`tadmm_svdconv_fwd`, the r-vector of a pixel stays in LDS), float32 and larger ranks as two `tadmm_tucker_1x1` launches
(`ops.svd_conv_pays`, measured: DESIGN.md section 7).  Other dtypes, float16 in grad mode, and SVDConv2dC with
padding != 0, take the reference composition.

Reference quirks kept on purpose (they are part of the contract of the state_dicts and model files):
  - SVDConv2dR checks `kernel_size != 1` / `stride != 1` on the RAW arguments, so `kernel_size=(1, 1)` raises.
  - SVDConv2dR from `dense_w` stores U in `left_factor` (O x r) and diag(s) V^T in `right_factor` (r x I): not the
    declared shapes (r x I, O x r), but `left_factor @ right_factor` is the weight.  Without `dense_w`,
    `reset_parameters` multiplies the declared (r x I) and (O x r) factors, which raises unless in == out.
  - SVDConv2dC / SVDConv2dM register `bias` twice: it comes first in the state_dict.
  - SVDConv2dC applies the padding to the second convolution only: the border of a padded output is the bias.
  - SVDConv2dM ignores the padding.  The reference returns a permuted (channels-last) view; here the kernel path returns
    a contiguous NCHW tensor with the same values.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import Tensor, nn
from torch.nn import init
from torch.nn.modules.utils import _pair

from . import functional as HF
from . import ops
from ._cabi import KIND_SVD
from ._layer_common import DenseConvMixin, make_bias


def svd_factors(ws, ranks, device=None):
    """Rank-r SVD factors of several 1x1 kernels / matrices in ONE device plan: [(U (O, r), diag(s) V^T (r, I))] as
    float32 device tensors.  `ws`: (O, I) or (O, I, 1, 1) tensors (the reference's `dense_w.squeeze()`)."""
    if device is None:
        cuda = [w for w in ws if w.is_cuda]
        device = cuda[0].device if cuda else torch.device("cuda", torch.cuda.current_device())
    layers = []
    for w, r in zip(ws, ranks):
        m = w.detach().to(device, torch.float32).reshape(w.shape[0], -1).contiguous()
        layers.append(dict(kind=KIND_SVD, W=m, U=torch.zeros_like(m), Z=torch.empty_like(m),
                           ranks=int(r if isinstance(r, int) else r[0])))
    plan = ops.ProjectionPlan(layers, want_cores=True)
    plan.run(update_u=False, use_u=False)
    out = []
    for i, L in enumerate(layers):
        c0, c1 = plan.core_tensors(i)                  # (1, O, r), (r, I, 1)
        o, i_ = L["W"].shape
        out.append((c0.reshape(o, -1).clone(), c1.reshape(-1, i_).clone()))
    plan.close()
    return out


def _rank_of(hp_dict, name):
    ranks = hp_dict.ranks[name]
    return ranks, (ranks if isinstance(ranks, int) else ranks[0])


class _SVDConvBase(HF.InferenceCacheMixin, nn.Module):
    def _setup(self, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, padding_mode, hp_dict,
               name):
        kernel_size, stride = _pair(kernel_size), _pair(stride)
        padding, dilation = _pair(padding), _pair(dilation)
        if padding_mode != 'zeros':
            raise ValueError("padding_mode must be zero in this mode")
        if groups != 1:
            raise ValueError("groups must be 1 in this mode")
        if kernel_size[0] * kernel_size[1] != 1:
            raise ValueError('kernel_size must be 1 in this mode')
        if stride[0] * stride[1] != 1:
            raise ValueError('stride must be 1')
        self.in_channels, self.out_channels = in_channels, out_channels
        self.ranks, self.rank = _rank_of(hp_dict, name)
        self.kernel_size, self.stride = kernel_size, stride
        self.padding, self.dilation = padding, dilation
        self.transposed = False
        self.output_padding = _pair(0)
        self.groups = groups
        self.padding_mode = padding_mode

    def _chain(self, x, w_in, w_out):
        """The layer on the kernel path: y = w_out (w_in x) + bias per pixel of an NCHW image."""
        r = w_in.shape[0]
        grad = torch.is_grad_enabled()
        cache = None if grad else self.__dict__.setdefault("_plane_cache", {})
        n = HF._nplanes(x)                            # (the plane cache keys on the plane dtype: planes_of)
        if ops.svd_conv_pays(x, r):
            planes = None if grad else (HF.planes_of(w_in, n, pad_rows=64, cache=cache, tag="in", like=x),
                                        HF.planes_of(w_out, n, pad_cols=64, cache=cache, tag="out", like=x))
            return HF.conv1x1_chain(x, w_in, w_out, self.bias, planes)
        p1 = None if grad else HF.planes_of(w_in, n, cache=cache, tag="in1", like=x)
        h = HF.pointwise(x, w_in, None, "tadmm_tucker_1x1", p1)
        p2 = None if grad else HF.planes_of(w_out, n, cache=cache, tag="out1", like=x)
        return HF.pointwise(h, w_out, self.bias, "tadmm_tucker_1x1", p2)

    def _kernel_ok(self, x):
        """float32 / bfloat16 images, and float16 ones for inference (grad mode keeps the reference composition)."""
        return x.is_cuda and x.dim() == 4 and HF.chain_dtype_ok(x, *self.parameters(recurse=False))


class SVDConv2dR(DenseConvMixin, _SVDConvBase):
    def __init__(self, in_channels: int, out_channels: int, kernel_size, stride=1, padding=0, dilation=1,
                 groups: int = 1, bias: bool = True, padding_mode: str = 'zeros', hp_dict=None, name: str = None,
                 dense_w: Tensor = None, dense_b: Tensor = None):
        if kernel_size != 1:                          # on the raw argument, as the reference: (1, 1) raises
            raise ValueError('kernel_size must be 1')
        if stride != 1:
            raise ValueError('stride must be 1')
        kernel_size, stride = _pair(kernel_size), _pair(stride)
        padding, dilation = _pair(padding), _pair(dilation)
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.ranks, self.rank = _rank_of(hp_dict, name)
        self.kernel_size, self.stride = kernel_size, stride
        self.padding, self.dilation = padding, dilation
        self._init_dense_conv(in_channels, out_channels, groups, padding_mode)
        self.transposed = False
        self.output_padding = _pair(0)
        self.groups = groups
        self.padding_mode = padding_mode
        self.left_factor = nn.Parameter(torch.empty(self.rank, self.in_channels))
        self.right_factor = nn.Parameter(torch.empty(self.out_channels, self.rank))
        make_bias(self, self.out_channels, bias, dense_b)
        if dense_w is not None:
            u, sv = svd_factors([dense_w], [self.rank])[0]
            self.left_factor.data = u                 # (O, r): the reference's layout, not the declared one
            self.right_factor.data = sv               # (r, I)
        else:
            self.reset_parameters()

    def reset_parameters(self):
        init.xavier_uniform_(self.left_factor)
        init.xavier_uniform_(self.right_factor)
        # the reference's product of the DECLARED shapes (r, I) x (O, r): raises unless in == out (kept, see module doc)
        weight = self.left_factor.mm(self.right_factor).unsqueeze(-1).unsqueeze(-1)
        if self.bias is not None:
            fan_in, _ = init._calculate_fan_in_and_fan_out(weight)
            bound = 1 / math.sqrt(fan_in)
            init.uniform_(self.bias, -bound, bound)

    def _recover_weight(self):
        if self.left_factor.is_cuda and self.left_factor.dtype == torch.float32:   # fp32 matrix cores (tadmm_gemm)
            return HF.mm(self.left_factor, self.right_factor).unsqueeze(-1).unsqueeze(-1)
        return self.left_factor.mm(self.right_factor).unsqueeze(-1).unsqueeze(-1)


class SVDConv2dC(_SVDConvBase):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 padding_mode='zeros', hp_dict=None, name=str, dense_w=None, dense_b=None):
        super().__init__()
        self._setup(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, padding_mode, hp_dict,
                    name)
        make_bias(self, self.out_channels, bias, dense_b)
        self.left_kernel = nn.Parameter(torch.empty(self.rank, self.in_channels, *self.kernel_size))
        self.right_kernel = nn.Parameter(torch.empty(self.out_channels, self.rank, *self.kernel_size))
        make_bias(self, self.out_channels, bias, dense_b)    # registered twice, as the reference: first in the state_dict
        if dense_w is not None:
            u, sv = svd_factors([dense_w], [self.rank])[0]
            self.right_kernel.data = u[:, :, None, None]
            self.left_kernel.data = sv[:, :, None, None]
        else:
            self.reset_parameters()

    def reset_parameters(self):
        init.xavier_uniform_(self.left_kernel)
        init.xavier_uniform_(self.right_kernel)

    def _reference(self, x):
        out = F.conv2d(x, self.left_kernel, None)
        return F.conv2d(out, self.right_kernel, self.bias, self.stride, self.padding, self.dilation, self.groups)

    def forward(self, x):
        if self.padding != (0, 0) or not self._kernel_ok(x):
            return self._reference(x)
        return self._chain(x, self.left_kernel.reshape(self.left_kernel.shape[0], -1),
                           self.right_kernel.reshape(self.right_kernel.shape[0], -1))

    def forward_flops(self, x):
        compr_params = (self.left_kernel.numel() + self.right_kernel.numel()) / 1000
        compr_flops = 0
        height_, width_ = x.shape[2], x.shape[3]           # the first (unpadded) 1x1 convolution keeps the plane
        compr_flops += height_ * width_ * self.left_kernel.numel() / 1000 / 1000
        out = self.forward(x)
        _, _, height_, width_ = out.shape
        compr_flops += height_ * width_ * self.right_kernel.numel() / 1000 / 1000
        base_params = self.kernel_size[0] * self.kernel_size[1] * self.in_channels * self.out_channels / 1000
        base_flops = height_ * width_ * self.kernel_size[0] * self.kernel_size[1] * \
            self.in_channels * self.out_channels / 1000 / 1000
        print('baseline # params: {:.2f}K\t compressed # params: {:.2f}K\t '
              'baseline # flops: {:.2f}M\t compressed # flops: {:.2f}M'.format(base_params, compr_params, base_flops,
                                                                               compr_flops))
        return out, base_flops, compr_flops

    def extra_repr(self) -> str:
        s = 'left_conv(in={}, out={}, kernel_size=(1, 1), bias=False), ' \
            'right_conv(in={}, out={}, kernel_size={}, stride={}, padding={}, bias={}), ' \
            .format(self.in_channels, self.rank,
                    self.rank, self.out_channels, self.kernel_size,
                    self.stride, self.padding, self.bias is None)
        return s


class SVDConv2dM(_SVDConvBase):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 padding_mode='zeros', hp_dict=None, name=str, dense_w=None, dense_b=None):
        super().__init__()
        self._setup(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, padding_mode, hp_dict,
                    name)
        make_bias(self, self.out_channels, bias, dense_b)
        self.left_factor = nn.Parameter(torch.empty(self.rank, self.in_channels))
        self.right_factor = nn.Parameter(torch.empty(self.out_channels, self.rank))
        make_bias(self, self.out_channels, bias, dense_b)    # registered twice, as the reference: first in the state_dict
        if dense_w is not None:
            u, sv = svd_factors([dense_w], [self.rank])[0]
            self.right_factor.data = u
            self.left_factor.data = sv
        else:
            self.reset_parameters()

    def reset_parameters(self):
        init.xavier_uniform_(self.left_factor)
        init.xavier_uniform_(self.right_factor)

    def forward(self, x):
        if not self._kernel_ok(x):                    # the reference composition (a channels-last view)
            out = F.linear(x.permute(0, 2, 3, 1), self.left_factor)
            return F.linear(out, self.right_factor, self.bias).permute(0, 3, 1, 2)
        return self._chain(x, self.left_factor, self.right_factor)
