"""Drop-in alias for `densenet_cifar_tt.py` (TenBasicBlock, TenBottleneckBlock, TenTransitionBlock, TenDenseBlock,
TenDenseNet and the `tkr_densenet40` factory): re-exports the MI355X-native implementation, which needs no timm.  The
factory takes the dense state dict as `dense_dict=` or from a local `path`; nothing is downloaded."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
from tadmm.densenet_cifar_layers import *  # noqa: E402,F401,F403
from tadmm.densenet_cifar_layers import FACTORIES, _ten_densenet  # noqa: E402,F401
