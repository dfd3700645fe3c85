"""Drop-in alias for `resnet_cifar_tt.py` (LambdaLayer, TTBasicBlock, TTResNet and the `ttr_` / `ttm_` / `tkr_` / `tkm_` /
`tkc_` / `stftkc_` factories of resnet20 / 32 / 56): re-exports the MI355X-native implementation, which needs no timm.  The
factories take the dense state dict as `dense_dict=` or from a local `path`; nothing is downloaded."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
from tadmm.resnet_cifar_layers import *  # noqa: E402,F401,F403
from tadmm.resnet_cifar_layers import FACTORIES, _tt_resnet  # noqa: E402,F401
