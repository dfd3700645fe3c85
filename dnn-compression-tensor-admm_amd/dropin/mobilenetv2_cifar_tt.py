"""Drop-in alias for `mobilenetv2_cifar_tt.py` (TTBaseBlock, TTMobileNetV2 and the `tkr_` / `tkc_` / `tkm_` / `svdr_` /
`svdc_` / `svdm_mobilenetv2_cifar` factories): re-exports the MI355X-native implementation, which needs no timm.  The
factories take the dense state dict as `dense_dict=` or from a local `path`; nothing is downloaded."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
from tadmm.mobilenet_cifar_layers import *  # noqa: E402,F401,F403
from tadmm.mobilenet_cifar_layers import FACTORIES, _tt_mobilenetv2_cifar  # noqa: E402,F401
