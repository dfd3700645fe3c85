"""Drop-in alias for `mobilenetv2_tt.py` (_make_divisible, conv_3x3_bn, conv_1x1_bn, tt_conv_1x1_bn, TTInvertedResidual,
TTMobileNetV2 and the `ttr_` / `tkc_` / `svdc_` / `svdm_mobilenetv2` factories): re-exports the MI355X-native
implementation, which needs no timm.  The factories take the dense state dict as `dense_dict=` or from a local `path`;
nothing is downloaded."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
from tadmm.mobilenet_inet_layers import *  # noqa: E402,F401,F403
from tadmm.mobilenet_inet_layers import FACTORIES, _make_divisible, _tt_mobilenetv2  # noqa: E402,F401
