"""Drop-in alias for `vit_tt.py` (TTAttention, TTMlp, TTBlock, TTVisionTransformer and the `tt{m,r}_` / `tk{m,r}_`
factories of vit_small / deit_tiny / deit_small): re-exports the MI355X-native implementation, which needs no timm.  The
factories take the dense state dict as `dense_dict=` or from a local `path`; nothing is downloaded."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
from tadmm.vit_layers import *  # noqa: E402,F401,F403
from tadmm.vit_layers import FACTORIES  # noqa: E402,F401
