"""The self-attention of a BERT encoder layer, as every `xcompression/transformer/compressed_modeling*.py` runs it:

    attn = BertSelfAttention(hidden_size, num_attention_heads, attention_probs_dropout_prob, linear=factory, layer_id=i)
    context_layer, attention_scores = attn(hidden_states, attention_mask)

The three projections are built by `linear(in_features, out_features)` (default `torch.nn.Linear`; a compressed model
passes a factory of `TTLinearM`) and are named `query`, `key`, `value` next to `dropout`, so the reference's state-dict
keys carry over.  Everything after them -- scores, mask, softmax, dropout and the context, with the raw masked scores as
a second differentiable output -- is `functional.self_attention`: one launch of csrc/attn.hip forward, two backward, or
the same arithmetic composed from torch operations where the launch does not take the call.

The rest of the encoder layer keeps the reference's class and attribute names, so its checkpoints load:

    layer = BertLayer(hidden_size, num_attention_heads, intermediate_size, ..., linear=factory, layer_id=i)
    layer_output, layer_att = layer(hidden_states, attention_mask)

`BertSelfOutput` and `BertOutput` end in LayerNorm(dropout(dense_out) + input_tensor), `BertLayerNorm` is the same
without a residual, `BertEmbeddings` normalises the sum of its three lookups: all four go through
`functional.residual_layer_norm` (csrc/bertnorm.hip: one launch forward, two backward).  `linear(in_features,
out_features)` builds every projection (default `torch.nn.Linear`); `TTLinear` has the fork's signature
(xcompression/transformer/TTLinear.py:138-194) on top of `tt_layers.TTLinearM`, and `reference_tt_linear` is the factory
with the shapes and ranks compressed_modeling_tt.py hard-wires.  The activation of `BertIntermediate` is torch's (one
launch each way, no bias to fold in), as are the embedding lookups, their two adds and the pooler's tanh."""
import types

import torch
import torch.nn.functional as F
from torch import nn

from . import functional as HF
from .tt_layers import TTLinearM

ACT2FN = {"gelu": F.gelu, "relu": F.relu}


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


class TTLinear(TTLinearM):
    """xcompression/transformer/TTLinear.py:138-223 on `TTLinearM`: `tt_shapes = out_shapes + in_shapes`, parameters
    `tt_cores.<i>` of shape (ranks[i], tt_shapes[i], ranks[i + 1]) and the same forward, which on a HIP device is the
    fused chain kernel where the middle rank fits it.  CPU tensors and float64 take the fork's chain of products in torch
    (there is no kernel for either).  `compression_ratio=` / `dim=` (shapes and ranks chosen automatically) are not
    carried over."""

    def __init__(self, in_features: int, out_features: int, bias: bool = False, ranks=None, in_shapes=None,
                 out_shapes=None, dense_w=None, dense_b=None, compression_ratio=None, dim=None):
        if compression_ratio is not None or dim is not None or ranks is None or in_shapes is None or out_shapes is None:
            raise NotImplementedError("TTLinear: compression_ratio= and dim= (automatic shapes and ranks) are not "
                                      "implemented; pass ranks=, in_shapes= and out_shapes=")
        tt_shapes = list(out_shapes) + list(in_shapes)
        hp = types.SimpleNamespace(tt_shapes={"w": tt_shapes}, ranks={"w": list(ranks)})
        super().__init__(in_features, out_features, bias=bias, hp_dict=hp, name="w", dense_w=dense_w, dense_b=dense_b)
        if self.out_tt_order != len(out_shapes):
            raise ValueError(f"TTLinear: out_shapes {list(out_shapes)} reach out_features {out_features} before their end")

    def forward(self, x):
        if not x.is_cuda or x.dtype == torch.float64:
            return self._forward_torch(x)
        return super().forward(x)

    def _forward_torch(self, x):                                 # TTLinear.py:206-223
        out_shape = list(x.shape)
        out_shape[-1] = self.out_features
        q = self.out_tt_order
        out = x
        for i in range(self.in_tt_order - 1, -1, -1):
            k = self.in_tt_shapes[i] * self.tt_ranks[i + q + 1]
            out = out.reshape(-1, k).mm(self.tt_cores[i + q].reshape(-1, k).t())
        for i in range(q - 1, -1, -1):
            r1 = self.tt_ranks[i + 1]
            out = self.tt_cores[i].reshape(-1, r1).mm(out.reshape(-1, r1).t())
            out = out.reshape(self.tt_ranks[i], -1).t()
        out = out.reshape(self.out_features, -1).t().reshape(out_shape)
        if self.bias is not None:
            out = out + self.bias
        return out


def reference_tt_linear(in_features: int, out_features: int):
    """The `linear=` factory with the shapes and ranks compressed_modeling_tt.py hard-wires for BERT-base: 768 -> 768
    (query, key, value, attention output) as [24, 32] -> [768] at rank 18, 768 -> 3072 as [768] -> [64, 48] at rank 18,
    3072 -> 768 as [48, 64] -> [768] at rank 17."""
    table = {(768, 768): ([24, 32], [768], [1, 18, 18, 1]), (768, 3072): ([768], [64, 48], [1, 18, 18, 1]),
             (3072, 768): ([48, 64], [768], [1, 17, 17, 1])}
    if (in_features, out_features) not in table:
        raise ValueError(f"reference_tt_linear: the reference has no TT shapes for {in_features} -> {out_features}")
    in_shapes, out_shapes, ranks = table[(in_features, out_features)]
    return TTLinear(in_features, out_features, in_shapes=in_shapes, out_shapes=out_shapes, ranks=ranks)


class BertLayerNorm(nn.Module):
    """compressed_modeling_tt.py:145-158: TF-style layer norm, epsilon inside the square root."""

    def __init__(self, hidden_size: int, eps: float = 1e-12):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.bias = nn.Parameter(torch.zeros(hidden_size))
        self.variance_epsilon = eps
        self.route = None

    def forward(self, x):
        return HF.residual_layer_norm(x, None, self.weight, self.bias, eps=self.variance_epsilon, route=self.route)


class _DenseDropNorm(nn.Module):
    """`dense`, then LayerNorm(dropout(.) + input_tensor): what BertSelfOutput and BertOutput share."""
    _hook = ""

    def __init__(self, in_features, hidden_size, hidden_dropout_prob, linear, layer_id, dense_first):
        super().__init__()
        self.layer_id = layer_id
        make = nn.Linear if linear is None else linear
        if dense_first:                         # registration order is the order of the reference's state-dict keys
            self.dense = make(in_features, hidden_size)
        self.LayerNorm = BertLayerNorm(hidden_size, eps=1e-12)
        self.dropout = nn.Dropout(hidden_dropout_prob)
        if not dense_first:
            self.dense = make(in_features, hidden_size)
        self.route = None                       # None: the measured rule; "launch" / "composed" force a route

    def forward(self, hidden_states, input_tensor, weights=None):
        if weights is not None:
            hidden_states = getattr(weights, self._hook)(hidden_states, self.layer_id)
        else:
            hidden_states = self.dense(hidden_states)
        return HF.residual_layer_norm(hidden_states, input_tensor, self.LayerNorm.weight, self.LayerNorm.bias,
                                      eps=self.LayerNorm.variance_epsilon, dropout_p=self.dropout.p,
                                      training=self.training, route=self.route)


class BertSelfOutput(_DenseDropNorm):
    """compressed_modeling_tt.py:420-440 (TTBertSelfOutput) and its siblings."""
    _hook = "output_transform"

    def __init__(self, hidden_size: int, hidden_dropout_prob: float = 0.1, linear=None, layer_id=None):
        super().__init__(hidden_size, hidden_size, hidden_dropout_prob, linear, layer_id, dense_first=False)


class BertOutput(_DenseDropNorm):
    """compressed_modeling_tt.py:471-494."""
    _hook = "ffn_output_transform"

    def __init__(self, intermediate_size: int, hidden_size: int, hidden_dropout_prob: float = 0.1, linear=None,
                 layer_id=None):
        super().__init__(intermediate_size, hidden_size, hidden_dropout_prob, linear, layer_id, dense_first=True)


class BertIntermediate(nn.Module):
    """compressed_modeling_tt.py:443-468: `dense`, then the activation ("gelu", "relu" or a callable; torch's)."""

    def __init__(self, hidden_size: int, intermediate_size: int, hidden_act="gelu", linear=None, layer_id=None):
        super().__init__()
        self.layer_id = layer_id
        make = nn.Linear if linear is None else linear
        self.dense = make(hidden_size, intermediate_size)
        self.intermediate_act_fn = ACT2FN[hidden_act] if isinstance(hidden_act, str) else hidden_act

    def forward(self, hidden_states, weights=None):
        if weights is not None:
            hidden_states = weights.ffn_inner_transform(hidden_states, self.layer_id)
        else:
            hidden_states = self.dense(hidden_states)
        return self.intermediate_act_fn(hidden_states)


class BertAttention(nn.Module):
    """compressed_modeling_tt.py:406-417."""

    def __init__(self, hidden_size: int, num_attention_heads: int, attention_probs_dropout_prob: float = 0.1,
                 hidden_dropout_prob: float = 0.1, linear=None, layer_id=None):
        super().__init__()
        self.layer_id = layer_id
        self.self = BertSelfAttention(hidden_size, num_attention_heads, attention_probs_dropout_prob, linear=linear,
                                      layer_id=layer_id)
        self.output = BertSelfOutput(hidden_size, hidden_dropout_prob, linear=linear, layer_id=layer_id)

    def forward(self, input_tensor, attention_mask):
        self_output, layer_att = self.self(input_tensor, attention_mask)
        attention_output = self.output(self_output, input_tensor)
        return attention_output, layer_att


class BertLayer(nn.Module):
    """compressed_modeling_tt.py:497-510.  `set_route` forces one route on the attention and both tails."""

    def __init__(self, hidden_size: int, num_attention_heads: int, intermediate_size: int, hidden_act="gelu",
                 hidden_dropout_prob: float = 0.1, attention_probs_dropout_prob: float = 0.1, linear=None, layer_id=None):
        super().__init__()
        self.attention = BertAttention(hidden_size, num_attention_heads, attention_probs_dropout_prob,
                                       hidden_dropout_prob, linear=linear, layer_id=layer_id)
        self.intermediate = BertIntermediate(hidden_size, intermediate_size, hidden_act, linear=linear, layer_id=layer_id)
        self.output = BertOutput(intermediate_size, hidden_size, hidden_dropout_prob, linear=linear, layer_id=layer_id)

    def set_route(self, route):
        for m in (self.attention.self, self.attention.output, self.output):
            m.route = route
        return self

    def forward(self, hidden_states, attention_mask):
        attention_output, layer_att = self.attention(hidden_states, attention_mask)
        intermediate_output = self.intermediate(attention_output)
        layer_output = self.output(intermediate_output, attention_output)
        return layer_output, layer_att


class BertEncoder(nn.Module):
    """compressed_modeling_tt.py:513-527: returns (the input and every layer's output, every layer's scores)."""

    def __init__(self, num_hidden_layers: int, hidden_size: int, num_attention_heads: int, intermediate_size: int,
                 hidden_act="gelu", hidden_dropout_prob: float = 0.1, attention_probs_dropout_prob: float = 0.1,
                 linear=None):
        super().__init__()
        self.layer = nn.ModuleList([
            BertLayer(hidden_size, num_attention_heads, intermediate_size, hidden_act, hidden_dropout_prob,
                      attention_probs_dropout_prob, linear=linear, layer_id=i) for i in range(num_hidden_layers)])

    def forward(self, hidden_states, attention_mask):
        all_encoder_layers = []
        all_encoder_atts = []
        for layer_module in self.layer:
            all_encoder_layers.append(hidden_states)
            hidden_states, layer_att = layer_module(hidden_states, attention_mask)
            all_encoder_atts.append(layer_att)
        all_encoder_layers.append(hidden_states)
        return all_encoder_layers, all_encoder_atts


class BertEmbeddings(nn.Module):
    """compressed_modeling_tt.py:288-336.  `word_embeddings` is the caller's module (`nn.Embedding` or one of
    `tadmm.emb_layers`); the three lookups and their two adds are torch's, the LayerNorm is
    `functional.residual_layer_norm`, the dropout comes after it."""

    def __init__(self, word_embeddings: nn.Module, max_position_embeddings: int, type_vocab_size: int, hidden_size: int,
                 hidden_dropout_prob: float = 0.1):
        super().__init__()
        self.word_embeddings = word_embeddings
        self.position_embeddings = nn.Embedding(max_position_embeddings, hidden_size)
        self.token_type_embeddings = nn.Embedding(type_vocab_size, hidden_size)
        self.LayerNorm = BertLayerNorm(hidden_size, eps=1e-12)
        self.dropout = nn.Dropout(hidden_dropout_prob)

    def get_weights(self):
        if type(self.word_embeddings) == nn.Embedding:
            return self.word_embeddings.weight
        return self.word_embeddings.get_weights()

    def forward(self, input_ids, token_type_ids=None):
        seq_length = input_ids.size(1)
        position_ids = torch.arange(seq_length, dtype=torch.long, device=input_ids.device)
        position_ids = position_ids.repeat(input_ids.shape[0], 1)
        if token_type_ids is None:
            token_type_ids = torch.zeros_like(input_ids)
        embeddings = self.word_embeddings(input_ids) + self.position_embeddings(position_ids) \
            + self.token_type_embeddings(token_type_ids)
        return self.dropout(self.LayerNorm(embeddings))


class BertPooler(nn.Module):
    """compressed_modeling_tt.py:530-548: `dense` on the first token of the last layer's output, then tanh."""

    def __init__(self, hidden_size: int):
        super().__init__()
        self.dense = nn.Linear(hidden_size, hidden_size)
        self.activation = nn.Tanh()

    def forward(self, hidden_states):
        return self.activation(self.dense(hidden_states[-1][:, 0]))
