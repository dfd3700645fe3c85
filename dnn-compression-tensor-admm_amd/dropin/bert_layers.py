"""Drop-in alias for the self-attention of `xcompression/transformer/compressed_modeling*.py`: re-exports the
MI355X-native implementation."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
from tadmm.bert_layers import BertSelfAttention  # noqa: E402,F401
