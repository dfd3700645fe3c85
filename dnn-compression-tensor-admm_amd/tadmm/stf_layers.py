"""Tucker-2 convolution whose two factor matrices live on the Stiefel manifold, with the reference's constructor
signature, errors and state_dict keys (StfTKConv.py:28-102).

  StfTKConv2dC : 1x1 conv -> k x k conv -> 1x1 conv          (first_kernel, core_kernel, last_kernel, bias)

    first_kernel (in_channels, in_rank)      note the orientation: transposed relative to TKConv2dC
    core_kernel  (out_rank, in_rank, kh, kw)
    last_kernel  (out_channels, out_rank)

The reference declares the two factors `geoopt.ManifoldParameter(manifold=geoopt.Stiefel())`; here they are
`StiefelParameter`s, an `nn.Parameter` subclass carrying `manifold = "stiefel"`, which `tadmm.riemannian.StiefelSGD`
selects on: their columns stay orthonormal through training (csrc/stiefel.hip).

The forward is `TKConv2dC`'s with w1 = first_kernel^T and w3 = last_kernel: the same fused, saved and float16-inference
routes, the same kernels on the same operand values.

Deliberate difference: `reset_parameters` does the reference's three `xavier_uniform_` calls and then PROJECTS the two
factors onto the manifold (the Q factor of their QR decomposition, positive diagonal of R).  The reference leaves them
off the manifold it declares.  The projection runs on the device; a module built on the CPU is projected when it is
moved to the device (`.to()` / `.cuda()`), unless a state_dict was loaded in between.

Second deliberate difference: a table rank above the channel count (`tk_resnet32_hp` 3x: in_rank 20 of the 16 input
channels of `layer2.0.conv1`) is clamped to the channel count, because no 16 x 20 matrix has orthonormal columns (the
reference builds a `ManifoldParameter` that cannot lie on its manifold).  `self.ranks` keeps the table's entry;
`in_rank` / `out_rank` and the parameter shapes carry the clamped values.
"""
from __future__ import annotations

import torch
from torch import Tensor, nn
from torch.nn import init

from . import ops
from ._layer_common import make_bias
from .tk_layers import _TKConvChain, _check_mode, _tucker_factors


class StiefelParameter(nn.Parameter):
    """An n x p parameter (n >= p) whose columns are kept orthonormal by `tadmm.riemannian.StiefelSGD`."""
    manifold = "stiefel"

    def __repr__(self):
        return "Stiefel parameter containing:\n" + torch.Tensor.__repr__(self.data)


class StfTKConv2dC(_TKConvChain):
    def __init__(self, in_channels: int, out_channels: int, kernel_size, stride=1, padding=0, dilation=1,
                 groups: int = 1, bias: bool = True, padding_mode: str = 'zeros', hp_dict=None, name: str = None,
                 dense_w: Tensor = None, dense_b: Tensor = None):
        _check_mode(groups, padding_mode)
        super().__init__()
        self._setup(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, padding_mode,
                    hp_dict.ranks[name])
        # no n x p matrix with p > n has orthonormal columns: a table rank above the channel count is clamped to it
        # (tk_resnet32_hp 3x lists in_rank 20 for the 16 input channels of layer2.0.conv1)
        self.in_rank, self.out_rank = min(self.in_rank, in_channels), min(self.out_rank, out_channels)
        self.first_kernel = StiefelParameter(torch.empty(self.in_channels, self.in_rank))
        self.core_kernel = nn.Parameter(torch.empty(self.out_rank, self.in_rank, *self.kernel_size))
        self.last_kernel = StiefelParameter(torch.empty(self.out_channels, self.out_rank))
        make_bias(self, self.out_channels, bias, dense_b)
        self._pending_projection = False
        if dense_w is not None:                       # the HOOI factors have orthonormal columns already
            core, u_out, u_in = _tucker_factors(dense_w, self.out_rank, self.in_rank)
            self.first_kernel.data = u_in.contiguous()
            self.last_kernel.data = u_out.contiguous()
            self.core_kernel.data = core
        else:
            self.reset_parameters()

    def reset_parameters(self) -> None:
        for p in (self.first_kernel, self.core_kernel, self.last_kernel):
            init.xavier_uniform_(p)
        self._pending_projection = True
        self._project_if_on_device()

    def project_(self) -> None:
        """Puts first_kernel and last_kernel on the manifold in place (device only)."""
        ops.stiefel_project_(self.first_kernel.detach(), self.last_kernel.detach())
        self._pending_projection = False
        self.invalidate_caches()

    def _project_if_on_device(self):
        if self._pending_projection and self.first_kernel.is_cuda and self.last_kernel.is_cuda \
                and self.first_kernel.dtype == torch.float32:
            self.project_()

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._project_if_on_device()
        return out

    def _load_from_state_dict(self, *args, **kwargs):
        self._pending_projection = False              # the loaded factors are the caller's
        return super()._load_from_state_dict(*args, **kwargs)

    def _factors(self):
        return self.first_kernel.t(), self.last_kernel
