"""Drop-in alias for the encoder layer of `xcompression/transformer/compressed_modeling*.py` (self-attention, the
dense + dropout + residual + LayerNorm tails, the feed-forward, the layer, the encoder, the embeddings, the pooler and
the fork's `TTLinear`): re-exports the MI355X-native implementation."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
from tadmm.bert_layers import (BertAttention, BertEmbeddings, BertEncoder, BertIntermediate, BertLayer,  # noqa: E402,F401
                               BertLayerNorm, BertOutput, BertPooler, BertSelfAttention, BertSelfOutput, TTLinear,
                               reference_tt_linear)
