"""TT-LSTM: the recurrent model of the paper's UCF11, YTC and TIMIT rows (ablation/tt_lstm_inference.py,
ablation/compare_tt_lstm.py).

  TTLSTM : tensor-train input-to-hidden map for all T*B tokens at once (an inner `TTLinearM`, one fused-chain launch
           where its middle rank allows), then the whole recurrence in ONE launch (csrc/lstm.hip)
           (keys i2h.tt_cores.i, h2h_weight, bias)

Gate order [i | f | g | o]; i, f, o go through Hardsigmoid like the reference's step function, or through the logistic
function (`gate="sigmoid"`) so that a model trained as `torch.nn.LSTM` and projected by ADMM can be loaded
(`TTLSTM.from_lstm`).
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import Tensor, nn
from torch.nn import init

from . import functional as HF
from ._cabi import TadmmError
from .tt_layers import TTLinearM


LONG_INPUT = 8192      # inputs above which the input map runs core by core (see TTLSTM.forward)


class _OneEntry:
    """The two tables of a rank table (`tt_shapes`, `ranks`) for one layer name."""

    def __init__(self, name, tt_shapes, ranks):
        self.tt_shapes, self.ranks = {name: list(tt_shapes)}, {name: list(ranks)}


class TTLSTM(nn.Module):
    def __init__(self, input_size: int, hidden_size: int, bias: bool = True, hp_dict=None, name: str = None,
                 dense_w_ih: Tensor = None, dense_w_hh: Tensor = None, dense_b: Tensor = None,
                 gate: str = "hardsigmoid", batch_first: bool = False):
        """`hp_dict.tt_shapes[name]` = [4 * o_0, o_1, .., i_0, ..] (tt_lstm_inference.py:31-32: the four gates multiply the
        first output mode), `hp_dict.ranks[name]` the rank list.  `dense_w_ih` (4H, in) is TT-decomposed on the device,
        `dense_w_hh` (4H, H) and `dense_b` (4H) are taken as they are."""
        if gate not in HF.LSTM_GATES:
            raise ValueError(f"TTLSTM: gate is 'hardsigmoid' or 'sigmoid' (got {gate!r})")
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        self.gate, self.batch_first = gate, batch_first
        self.i2h = TTLinearM(input_size, 4 * hidden_size, bias=False, hp_dict=hp_dict, name=name, dense_w=dense_w_ih)
        self.h2h_weight = nn.Parameter(torch.empty(4 * hidden_size, hidden_size))
        if bias:
            self.bias = nn.Parameter(torch.empty(4 * hidden_size))
        else:
            self.register_parameter("bias", None)
        bound = 1.0 / math.sqrt(hidden_size)
        init.uniform_(self.h2h_weight, -bound, bound)
        if dense_w_hh is not None:
            if tuple(dense_w_hh.shape) != (4 * hidden_size, hidden_size):
                raise ValueError(f"TTLSTM: dense_w_hh must be ({4 * hidden_size}, {hidden_size})")
            self.h2h_weight.data = dense_w_hh.detach().clone().float()
        if self.bias is not None:
            init.uniform_(self.bias, -bound, bound)
            if dense_b is not None:
                if tuple(dense_b.shape) != (4 * hidden_size,):
                    raise ValueError(f"TTLSTM: dense_b must be ({4 * hidden_size},)")
                self.bias.data = dense_b.detach().clone().float()

    @classmethod
    def from_lstm(cls, lstm: nn.LSTM, hp_dict, name: str) -> "TTLSTM":
        """A single-layer, unidirectional `torch.nn.LSTM` as a TTLSTM: `weight_ih_l0` is TT-decomposed with the shapes and
        ranks of `hp_dict` (after ADMM on that weight the decomposition is exact to rounding), `weight_hh_l0` copied, the
        two biases summed, the gates logistic.  ValueError for anything else (layers, directions, projections)."""
        if not isinstance(lstm, nn.LSTM):
            raise ValueError(f"TTLSTM.from_lstm: a torch.nn.LSTM is required (got {type(lstm).__name__})")
        if lstm.num_layers != 1 or lstm.bidirectional or getattr(lstm, "proj_size", 0):
            raise ValueError("TTLSTM.from_lstm: one layer, one direction and no projection "
                             f"(got num_layers={lstm.num_layers}, bidirectional={lstm.bidirectional}, "
                             f"proj_size={getattr(lstm, 'proj_size', 0)})")
        b = (lstm.bias_ih_l0.detach() + lstm.bias_hh_l0.detach()) if lstm.bias else None
        return cls(lstm.input_size, lstm.hidden_size, bias=lstm.bias, hp_dict=hp_dict, name=name,
                   dense_w_ih=lstm.weight_ih_l0.detach(), dense_w_hh=lstm.weight_hh_l0.detach(), dense_b=b,
                   gate="sigmoid", batch_first=lstm.batch_first)

    def get_ranks(self):
        return ', '.join(str(r) for r in self.i2h.tt_ranks)

    def compression_ratio(self) -> float:
        """tt_lstm_inference.py:28-41: the dense input map's 4 * in * H parameters over the cores' (the recurrent weight
        and the bias are on neither side)."""
        return 4 * self.input_size * self.hidden_size / sum(p.numel() for p in self.i2h.tt_cores)

    def forward_flops(self, batch_size: int = 1):
        """(dense, tt) multiply-adds of the input map for `batch_size` tokens, counted as compare_tt_lstm.py:64,77-92
        does: every core product as rows x reduction x columns."""
        m = self.i2h
        q, r = m.out_tt_order, m.tt_ranks
        numel, tt = batch_size * self.input_size, 0
        for i in range(m.in_tt_order - 1, -1, -1):
            k = m.in_tt_shapes[i] * r[i + q + 1]
            cols = numel // k
            tt += r[i + q] * k * cols
            numel = r[i + q] * cols
        for i in range(q - 1, -1, -1):
            cols = numel // r[i + 1]
            tt += r[i] * m.out_tt_shapes[i] * r[i + 1] * cols
            numel = r[i] * m.out_tt_shapes[i] * cols
        return batch_size * self.input_size * 4 * self.hidden_size, tt

    def forward(self, x: Tensor, state=None, route: str = None):
        """x (T, B, in) -- (B, T, in) with `batch_first` -- float32 -> (y (T, B, H), (h_T, c_T)); `state` = (h_0, c_0),
        (B, H) each, zeros when None."""
        if x.dim() != 3 or x.shape[-1] != self.input_size:
            raise ValueError(f"TTLSTM: x must be (T, B, {self.input_size}) (got {tuple(x.shape)})")
        if x.dtype != torch.float32:
            raise TadmmError(-1, f"TTLSTM: x must be float32 (got {x.dtype}); the recurrence has no bfloat16 / float16 form")
        if self.batch_first:
            x = x.transpose(0, 1)
        T, B = x.shape[0], x.shape[1]
        x2 = x.reshape(T * B, self.input_size)
        # The contracted chain sums all `input_size` products of an output into ONE float32 accumulator, 32 per MFMA: a
        # random walk of sqrt(in / 32) roundings, which passes float32 arithmetic's own error (about 1e-6 of the largest
        # entry) near 8192 inputs.  The long input maps (UCF11 / YTC: 57 600) therefore keep the reference's per-core
        # products, whose reductions are n_k r_k long; it is still one pass over all T*B tokens.
        xp = self.i2h._forward_chain(x2) if self.input_size > LONG_INPUT else self.i2h(x2)
        if self.bias is not None:
            xp = xp + self.bias
        h0, c0 = (None, None) if state is None else state
        y, (hT, cT) = HF.lstm_sequence(xp.reshape(T, B, 4 * self.hidden_size), self.h2h_weight, h0, c0, self.gate, route)
        return (y.transpose(0, 1) if self.batch_first else y), (hT, cT)


def entry(name: str, tt_shapes, ranks) -> _OneEntry:
    """A one-layer rank table for `TTLSTM(..., hp_dict=entry(name, tt_shapes, ranks), name=name)`."""
    return _OneEntry(name, tt_shapes, ranks)
