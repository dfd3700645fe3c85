"""Drop-in alias of the reference module `StfTKConv.py`: re-exports the MI355X-native implementation.  The optimiser
that replaces `geoopt.optim.RiemannianSGD` for these layers is `tadmm.riemannian.StiefelSGD`."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
from tadmm.stf_layers import StfTKConv2dC, StiefelParameter  # noqa: E402,F401
