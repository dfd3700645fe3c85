"""Drop-in alias of the reference module `SVDConv.py`: re-exports the MI355X-native implementation."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
from tadmm.svd_layers import SVDConv2dC, SVDConv2dM, SVDConv2dR  # noqa: E402,F401
