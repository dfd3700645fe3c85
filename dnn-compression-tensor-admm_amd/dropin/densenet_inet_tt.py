"""Drop-in alias for `densenet_inet_tt.py` (TenDenseLayer, TenDenseBlock, TenDenseTransition, TenDenseNet and the
`tkc_densenet121` / `tkc_densenet201` / `tkc_densenet264` factories): re-exports the MI355X-native implementation, which
needs no timm.  The factories take the dense state dict as `dense_dict=` or from a local `path`; nothing is downloaded."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
from tadmm.densenet_inet_layers import *  # noqa: E402,F401,F403
from tadmm.densenet_inet_layers import FACTORIES, _ten_densenet  # noqa: E402,F401
