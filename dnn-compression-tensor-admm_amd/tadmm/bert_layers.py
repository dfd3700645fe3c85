"""The self-attention of a BERT encoder layer, as every `xcompression/transformer/compressed_modeling*.py` runs it:

    attn = BertSelfAttention(hidden_size, num_attention_heads, attention_probs_dropout_prob, linear=factory, layer_id=i)
    context_layer, attention_scores = attn(hidden_states, attention_mask)

The three projections are built by `linear(in_features, out_features)` (default `torch.nn.Linear`; a compressed model
passes a factory of `TTLinearM`) and are named `query`, `key`, `value` next to `dropout`, so the reference's state-dict
keys carry over.  Everything after them -- scores, mask, softmax, dropout and the context, with the raw masked scores as
a second differentiable output -- is `functional.self_attention`: one launch of csrc/attn.hip forward, two backward, or
the same arithmetic composed from torch operations where the launch does not take the call."""
import torch
from torch import nn

from . import functional as HF


class BertSelfAttention(nn.Module):
    """compressed_modeling_tt.py:340-403 (TTBertSelfAttention) and its siblings."""

    def __init__(self, hidden_size: int, num_attention_heads: int, attention_probs_dropout_prob: float = 0.1,
                 linear=None, layer_id=None):
        super().__init__()
        self.layer_id = layer_id
        if hidden_size % num_attention_heads != 0:
            raise ValueError(
                "The hidden size (%d) is not a multiple of the number of attention "
                "heads (%d)" % (hidden_size, num_attention_heads))
        self.num_attention_heads = num_attention_heads
        self.attention_head_size = int(hidden_size / num_attention_heads)
        self.all_head_size = self.num_attention_heads * self.attention_head_size
        make = nn.Linear if linear is None else linear
        self.query = make(hidden_size, self.all_head_size)
        self.key = make(hidden_size, self.all_head_size)
        self.value = make(hidden_size, self.all_head_size)
        self.dropout = nn.Dropout(attention_probs_dropout_prob)
        self.route = None                       # None: the measured rule; "launch" / "composed" force a route

    def forward(self, hidden_states, attention_mask, output_att=False, weights=None):
        if weights is not None:
            q, k, v = weights.qkv_transform(hidden_states, self.layer_id)
        else:
            q = self.query(hidden_states)
            k = self.key(hidden_states)
            v = self.value(hidden_states)
        context_layer, attention_scores = HF.self_attention(
            q, k, v, attention_mask, self.num_attention_heads, dropout_p=self.dropout.p, training=self.training,
            need_scores=True, route=self.route)
        return context_layer, attention_scores
