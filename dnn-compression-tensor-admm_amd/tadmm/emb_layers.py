"""Factorised embedding tables with the reference's constructor signatures, attribute names and state_dict keys
(xcompression/transformer/TTEmbedding.py, TTMEmbedding.py, SVDEmbedding.py).

  TTMEmbedding : cores.k (r_k, n_k, m_k, r_{k+1});  row t = product of the slices the split index picks
  TTEmbedding  : cores.k (r_k, s_k, r_{k+1}) over input_tt_shape + output_tt_shape; the input cores are gathered to a
                 (tokens, r) matrix, which multiplies the tail rebuilt from the output cores
  SVDEmbedding : first_factor (num_embeddings, rank), last_factor (rank, embedding_dim); rows of first_factor are
                 gathered and multiply last_factor

All three look rows up through `functional.ttm_embedding`: one launch of the gathered TT-matrix chain
(csrc/ttm_gather.hip) instead of the reference's div / fmod / index_select / bmm sequence, with its own backward; the
dense products behind it are `functional.mm`.  Which calls take the launch is the measured rule `ops.ttm_gather_pays`
(DESIGN.md section 16): every call without gradients, and one-mode tables up to 512 tokens with them; the others, and
shapes beyond the LDS of a CU, run the same steps as torch ops on the device.  An index outside the table gives a zero
row and no gradient and is counted in `bad_index_count` (one int32 on the device, not part of the state_dict; reading
it is the only synchronisation), where the reference's `index_select` raises.

Not carried over:
  - `TTMEmbedding.initialize`: it cannot run in the reference (it hands tensors to the constructor of `MSELoss`).
  - `TTEmbedding.forward2`, an unused variant that skips all output cores but the last.
  - a single input mode (`len(input_tt_shape) == 1`) for TTEmbedding / TTMEmbedding: the reference's index split yields
    two index columns for one core there; a ValueError says so.  SVDEmbedding is the one-mode table.
  - tt_ranks[0] != 1 or tt_ranks[-1] != 1 (the reference's TTMEmbedding takes a trace over them): ValueError.

Deviations, stated where they apply: every forward returns input.shape + (size,) (the reference's TTMEmbedding
flattens the index and returns (tokens, size); the values and their order are the same); `init_pretrained_emb` runs
the device TT-SVD (`ttd.ten2tt`) and zero-pads a table that has fewer rows than prod(input_tt_shape);
`restore_weights` uses `output_size` where the reference hard-codes 16; `tt2ten` and `restore_weights` return device
tensors; a missing rank argument and a compression ratio no rank scale serves raise ValueError (the reference asserts).
"""
from __future__ import annotations

import math

import torch
from torch.nn import Module, Parameter, ParameterList, init

from . import functional as HF
from . import ttd
from .svd_layers import svd_factors
from .tt_layers import _chain_recover


def compute_ranks_tt(tt_shapes, ratio):
    """TT ranks [1, r, .., r, 1] of a tensor with modes `tt_shapes` at compression `ratio`.  A TT with one inner rank r
    holds inner * r^2 + outer * r values (outer: the two end modes, inner: the sum of the others); r is the positive
    root of inner r^2 + outer r = prod / ratio, rounded down.  Two modes hold r * (n_1 + n_2) values."""
    sizes = [int(v) for v in tt_shapes]
    budget = math.prod(sizes) / ratio
    if len(sizes) == 2:
        return [1, int(math.prod(sizes) / (ratio * sum(sizes))), 1]
    outer, inner = sizes[0] + sizes[-1], sum(sizes[1:-1])
    rank = int((math.sqrt(outer * outer + 4 * inner * budget) - outer) / (2 * inner))
    return [1, *([rank] * (len(sizes) - 1)), 1]


def _index_factors(modes):
    """Strides of all input modes but the last in the row index (i_1 slowest): the products of the modes after each."""
    return [math.prod(modes[k + 1:]) for k in range(len(modes) - 1)]


def _check_modes(who, input_tt_shape, tt_ranks):
    if len(input_tt_shape) < 2:
        raise ValueError(f"{who}: len(input_tt_shape) == 1 is not supported: the reference's index split produces two "
                         "index columns for one mode there; use SVDEmbedding for a one-mode table")
    if tt_ranks[0] != 1 or tt_ranks[-1] != 1:
        raise ValueError(f"{who}: tt_ranks must begin and end with 1 (got {list(tt_ranks)})")


class _EmbBase(Module):
    def _make_counter(self):
        self.register_buffer("bad_index_count", torch.zeros(1, dtype=torch.int32), persistent=False)

    def _xavier(self, tensors):
        for t in tensors:
            init.xavier_uniform_(t)


class TTMEmbedding(_EmbBase):
    def __init__(self, input_tt_shape, output_tt_shape, tt_ranks):
        super().__init__()
        if len(output_tt_shape) != len(input_tt_shape) or len(tt_ranks) != len(input_tt_shape) + 1:
            raise ValueError("TTMEmbedding: input_tt_shape, output_tt_shape and tt_ranks[:-1] must have one length")
        _check_modes("TTMEmbedding", input_tt_shape, tt_ranks)
        self.input_tt_shape, self.output_tt_shape, self.tt_ranks = input_tt_shape, output_tt_shape, tt_ranks
        self.n_dim = len(input_tt_shape)
        self.output_size = math.prod(output_tt_shape)
        self.tt_index_factor = _index_factors(input_tt_shape)
        shapes = zip(tt_ranks[:-1], input_tt_shape, output_tt_shape, tt_ranks[1:])
        self.cores = ParameterList([Parameter(torch.empty(*shape)) for shape in shapes])
        self._make_counter()
        self.reset_parameters()

    def get_core_size(self):
        return sum(int(c.numel()) for c in self.cores)

    def get_tt_ranks(self):
        return ", ".join(map(str, self.tt_ranks))

    def reset_parameters(self):
        self._xavier(self.cores)

    def compute_ranks_ttm(self, ratio):
        """TT-matrix ranks at compression `ratio`, the reference's rule restated.  With s_k = n_k m_k and T = prod s_k:
        cap_k = min(cap_{k-1} s_k, T / (s_1 ... s_k)) is the largest rank boundary k can carry.  The first cap is kept
        and the caps behind it are scaled by one factor x in (0, 1): with c the values of the two end cores minus T /
        ratio, b the values of the second and the second-last core and a those of the cores between, x = -c / b when
        a = 0 and the positive root of a x^2 + b x + c = 0 otherwise.  Each rank is then cut to min(r_{k-1} s_k, T /
        (r_{k-1} s_k)).  ValueError when x leaves (0, 1)."""
        sizes = [int(n) * int(m) for n, m in zip(self.input_tt_shape, self.output_tt_shape)]
        modes, total = len(sizes), math.prod(sizes)
        rest, caps = total, []
        for k in range(modes - 1):
            rest = rest / sizes[k]
            caps.append(int(min((caps[-1] if caps else 1) * sizes[k], rest)))
        ends = sizes[0] * caps[0] + sizes[-1] * caps[-1] - total / ratio
        seconds = sizes[1] * caps[1] * caps[0] + sizes[-2] * caps[-1] * caps[-2]
        middle = sum(caps[k - 1] * caps[k] * sizes[k] for k in range(2, modes - 2))
        if middle == 0:
            scale = -ends / seconds
        else:
            scale = (math.sqrt(seconds ** 2 - 4 * middle * ends) - seconds) / (2 * middle)
        if not 0 < scale < 1:
            raise ValueError(f"compute_ranks_ttm: no rank scale in (0, 1) gives ratio {ratio} (got {scale})")
        ranks = [1, caps[0], *(int(cap * scale) for cap in caps[1:]), 1]
        for k in range(modes - 1):
            rows = ranks[k] * sizes[k]
            ranks[k + 1] = int(min(ranks[k + 1], rows, total / rows))
        return ranks

    def forward(self, input):
        return HF.ttm_embedding(list(self.cores), input, self.bad_index_count)


class TTEmbedding(_EmbBase):
    def __init__(self, input_tt_shape, output_tt_shape, tt_ranks=None, compression_ratio=None):
        super().__init__()
        if compression_ratio is None and tt_ranks is None:
            raise ValueError("TTEmbedding: give tt_ranks or compression_ratio")
        self.tt_shapes = input_tt_shape + output_tt_shape
        self.tt_ranks = tt_ranks if compression_ratio is None else compute_ranks_tt(self.tt_shapes, compression_ratio)
        _check_modes("TTEmbedding", input_tt_shape, self.tt_ranks)
        if len(self.tt_ranks) != len(self.tt_shapes) + 1:
            raise ValueError("TTEmbedding: tt_ranks wants len(input_tt_shape) + len(output_tt_shape) + 1 entries")
        self.input_tt_shape, self.output_tt_shape = input_tt_shape, output_tt_shape
        self.output_size = math.prod(output_tt_shape)
        self.tt_index_factor = _index_factors(input_tt_shape)
        shapes = zip(self.tt_ranks[:-1], self.tt_shapes, self.tt_ranks[1:])
        self.cores = ParameterList([Parameter(torch.empty(*shape)) for shape in shapes])
        self._make_counter()
        self.reset_parameters()

    def get_core_size(self):
        return sum(int(c.numel()) for c in self.cores)

    def get_tt_ranks(self):
        return ", ".join(map(str, self.tt_ranks))

    def reset_parameters(self):
        self._xavier(self.cores)

    def forward(self, input):
        din = len(self.input_tt_shape)
        rows = HF.ttm_embedding([c.unsqueeze(2) for c in self.cores[:din]], input, self.bad_index_count)
        r = rows.shape[-1]
        tail = _chain_recover(list(self.cores[din:])).reshape(r, self.output_size)
        out = HF.mm(rows.reshape(-1, r), tail)
        return out.reshape(tuple(input.shape) + (self.output_size,))

    def init_pretrained_emb(self, emb):
        """TT-SVD of a pretrained table into the cores (TTEmbedding.py:143-168), on the device (`ttd.ten2tt`, the
        decomposition of the ADMM projection) where the reference runs LAPACK on the host.  Deviation: a table with
        fewer rows than prod(input_tt_shape) is zero-padded to that many rows (the reference's reshape fails); with
        matching sizes the cores span the same table as the reference's, up to the sign of each singular pair."""
        rows = math.prod(self.input_tt_shape)
        t = emb.detach().to(torch.float32)
        if t.dim() != 2 or t.shape[1] != self.output_size or t.shape[0] > rows:
            raise ValueError(f"init_pretrained_emb: a table of at most {rows} rows of {self.output_size} values "
                             f"(got {tuple(t.shape)})")
        dev = t.device if t.is_cuda else self.cores[0].device
        if dev.type != "cuda":
            dev = torch.device("cuda", torch.cuda.current_device())
        t = t.to(dev)
        if t.shape[0] < rows:
            t = torch.cat([t, t.new_zeros(rows - t.shape[0], t.shape[1])], 0)
        cores = ttd.ten2tt(t.contiguous(), list(self.tt_shapes), list(self.tt_ranks))
        for i, c in enumerate(cores):
            self.cores[i].data = c.to(self.cores[i].device)

    def restore_weights(self):
        """The dense (prod(input_tt_shape), output_size) table, differentiable (the reference's view(-1, 16) with
        `output_size` in place of 16)."""
        return _chain_recover(list(self.cores)).reshape(-1, self.output_size)

    def tt2ten(self):
        return _chain_recover([c.detach() for c in self.cores]).reshape(list(self.tt_shapes))


class SVDEmbedding(_EmbBase):
    def __init__(self, num_embeddings, embedding_dim, rank=None, compression_ratio=None, weights=None):
        super().__init__()
        if compression_ratio is None and rank is None:
            raise ValueError("SVDEmbedding: give rank or compression_ratio")
        self.num_embeddings, self.embedding_dim = num_embeddings, embedding_dim
        # a rank-r pair holds r * (rows + columns) values: the largest r within dense / ratio
        dense, per_rank = num_embeddings * embedding_dim, num_embeddings + embedding_dim
        self.rank = rank if compression_ratio is None else int(dense / (compression_ratio * per_rank))
        self.first_factor = Parameter(torch.empty(num_embeddings, self.rank))
        self.last_factor = Parameter(torch.empty(self.rank, embedding_dim))
        self._make_counter()
        if weights is None:
            self.reset_parameters()
        else:
            # one-layer device SVD plan (ops.ProjectionPlan, KIND_SVD, want_cores=True), as svd_layers.py: U and
            # diag(s) V^T, the reference's factors up to the sign of each singular pair
            self.first_factor.data, self.last_factor.data = svd_factors([weights], [self.rank])[0]

    def reset_parameters(self):
        self._xavier((self.first_factor, self.last_factor))

    def forward(self, x):
        core = self.first_factor.reshape(1, self.num_embeddings, 1, self.first_factor.shape[1])
        rows = HF.ttm_embedding([core], x, self.bad_index_count)
        out = HF.mm(rows.reshape(-1, rows.shape[-1]), self.last_factor)
        return out.reshape(tuple(x.shape) + (self.embedding_dim,))
