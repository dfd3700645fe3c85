"""Drop-in alias for `resnet_inet_tt.py` (tt_conv3x3, tt_conv1x1, TTBasicBlock, TTBottleneck, TTResNet and the eleven
`ttr_` / `ttm_` / `tkc_` / `tkm_` / `tkr_` factories of resnet18 / 34 / 50): re-exports the MI355X-native implementation,
which needs no timm.  The factories take the dense state dict as `dense_dict=` or from a local `path`; nothing is
downloaded."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
from tadmm.resnet_inet_layers import *  # noqa: E402,F401,F403
from tadmm.resnet_inet_layers import FACTORIES, _tt_resnet  # noqa: E402,F401
