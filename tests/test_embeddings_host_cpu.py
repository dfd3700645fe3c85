"""Host-side checks of the factorised embeddings: index split and grouping, the LDS fit arithmetic, the descriptor
layout, the rank helpers against the reference's recorded values, the argument errors, and how far a float32
restatement of the operation is from float64 at the shapes the GPU tests run.  No GPU needed."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import _emb_ref as R
from tadmm import _cabi, emb_layers, ops
from tadmm import functional as HF


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "g10_embeddings.json")))


@pytest.mark.parametrize("n", [[7], [3, 2], [4, 3, 5], [3, 2, 2, 3], [32, 31, 31]])
def test_index_split_and_groups(n):
    total = int(np.prod(n))
    rng = np.random.default_rng(1)
    idx = rng.integers(0, total, size=97)
    idx[0], idx[-1] = 0, total - 1
    t = torch.from_numpy(idx)
    split = torch.stack(ops.ttm_index_split(t, n), 1).numpy()
    assert np.array_equal(split, R.split_index(idx, n))
    # i_1 slowest: the mode indices rebuild the index
    strides = [int(np.prod(n[k + 1:])) for k in range(len(n))]
    assert np.array_equal(split @ np.array(strides), idx)
    for (order, offs), (order_ref, offs_ref) in zip(ops.ttm_groups(t.to(torch.int32), n), R.groups(idx, n)):
        assert np.array_equal(order.numpy(), order_ref) and np.array_equal(offs.numpy(), offs_ref)
        assert offs.shape[0] == len(offs_ref) and int(offs[-1]) == idx.size


def test_groups_put_bad_indices_in_range():
    n = [4, 3, 5]
    idx = torch.tensor([-1, 5, 60, 59, 0, -7, 61])
    for k, (order, offs) in enumerate(ops.ttm_groups(idx, n)):
        assert sorted(order.tolist()) == list(range(7)) and offs.shape[0] == n[k] + 1
        assert int(offs[0]) == 0 and int(offs[-1]) == 7


def test_fits_arithmetic():
    for name, (n, m, r) in R.SHAPES.items():
        fits, nbytes, tile = ops.ttm_gather_plan(n, m, r)
        fwd_token, bwd = R.lds_bytes(n, m, r)
        assert 1 <= tile <= 16
        assert nbytes == max(256 + tile * fwd_token, bwd), name
        assert fits == (nbytes <= ops.TTM_LDS_BYTES), name
        assert ops.ttm_gather_fits(n, m, r) == fits
    assert ops.ttm_gather_plan(*R.SHAPES["lds_last_fit"])[:2] == (True, 163088)
    assert ops.ttm_gather_plan(*R.SHAPES["lds_past"])[:2] == (False, 167440)
    assert ops.ttm_gather_plan(*R.SHAPES["bert_ttm"]) == (True, 16 + 4 * (684 + 5472 + 2 * 3648 + 5472), 1)
    assert ops.ttm_gather_plan(*R.SHAPES["svd_row"])[2] == 16          # short rows: 16 tokens per workgroup
    # sizes beyond 32-bit indexing are refused without being sized
    assert ops.ttm_gather_plan([2, 2], [40000, 40000], [1, 2, 1]) == (False, 0, 0)
    assert ops.ttm_gather_plan([70000], [1], [1, 40000]) == (False, 0, 0)
    # five modes never take the launch; the composed route serves them
    assert ops.ttm_gather_fits([2] * 5, [2] * 5, [1, 2, 2, 2, 2, 1]) is False


def test_routing_rule():
    """`ops.ttm_gather_pays` as measured: inference always on the launch; with gradients one mode up to 512 tokens."""
    bert = R.SHAPES["bert_ttm"]
    assert ops.ttm_gather_pays(*bert, 4096) and ops.ttm_gather_pays(*bert, 1, grad=False)
    assert not ops.ttm_gather_pays(*bert, 512, grad=True) and not ops.ttm_gather_pays(*bert, 1, grad=True)
    one = ([30522], [1], [1, 128])
    assert ops.ttm_gather_pays(*one, 512, grad=True) and not ops.ttm_gather_pays(*one, 513, grad=True)
    with pytest.raises(ValueError, match="route"):
        HF.ttm_embedding([torch.zeros(1, 3, 2, 1)], torch.zeros(3, dtype=torch.int64), route="fast")


def test_descriptor_size():
    lib = _cabi.load()
    assert lib.tadmm_ttm_desc_bytes() == C.sizeof(_cabi.TtmDesc)
    assert C.sizeof(_cabi.TtmDesc) == 4 * 4 * 8 + 4 * 8 + 8 + 2 * 4 + (4 + 4 + 5) * 4 + 4
    d = _cabi.TtmDesc()
    d.d = 0
    assert lib.tadmm_ttm_gather_fits(C.byref(d), None, None) == -1
    d.d, d.n[0], d.m[0], d.r[0], d.r[1] = 1, 3, 2, 2, 1
    assert lib.tadmm_ttm_gather_fits(C.byref(d), None, None) == -1     # r_0 != 1
    d.r[0] = 1
    assert lib.tadmm_ttm_gather_fits(C.byref(d), None, None) == 1


def test_rank_helpers_match_reference(golden):
    assert golden["ranks_tt"] and golden["ranks_ttm"]
    for e in golden["ranks_tt"]:
        assert emb_layers.compute_ranks_tt(e["tt_shapes"], e["ratio"]) == e["ranks"]
    for e in golden["ranks_ttm"]:
        layer = emb_layers.TTMEmbedding(e["input_tt_shape"], e["output_tt_shape"], [1] * (len(e["input_tt_shape"]) + 1))
        assert layer.compute_ranks_ttm(e["ratio"]) == e["ranks"]


def test_state_dict_keys_and_helpers(golden):
    for key, c in golden["cases"].items():
        if c["cls"] == "TTM":
            layer = emb_layers.TTMEmbedding(c["input_tt_shape"], c["output_tt_shape"], c["tt_ranks"])
        elif c["cls"] == "TT":
            layer = emb_layers.TTEmbedding(c["input_tt_shape"], c["output_tt_shape"], tt_ranks=c["tt_ranks"])
        else:
            layer = emb_layers.SVDEmbedding(c["num_embeddings"], c["embedding_dim"], rank=c["rank"])
        assert [[k, list(v.shape)] for k, v in layer.state_dict().items()] == c["state_dict"], key
        if c["cls"] != "SVD":
            assert layer.get_core_size() == sum(int(np.prod(s)) for _, s in c["state_dict"])
            assert layer.get_tt_ranks() == ", ".join(str(v) for v in c["tt_ranks"])
    layer = emb_layers.TTEmbedding([13, 13, 13, 14], [8, 4, 4, 6], compression_ratio=5)
    assert layer.tt_ranks == [1] + [290] * 7 + [1] and layer.tt_index_factor == [13 * 13 * 14, 13 * 14, 14]
    assert emb_layers.SVDEmbedding(30522, 768, compression_ratio=5).rank == 149


def test_argument_errors():
    with pytest.raises(ValueError, match="two index columns"):
        emb_layers.TTMEmbedding([12], [8], [1, 1])
    with pytest.raises(ValueError, match="two index columns"):
        emb_layers.TTEmbedding([30522], [768], compression_ratio=5)
    with pytest.raises(ValueError, match="begin and end with 1"):
        emb_layers.TTMEmbedding([3, 2], [2, 3], [2, 5, 2])
    idx = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="d = 0"):
        HF.ttm_embedding([], idx)
    with pytest.raises(ValueError, match="d = 0"):
        ops.ttm_gather_fits([], [], [1])
    with pytest.raises(ValueError, match="r_0 must be 1"):
        HF.ttm_embedding([torch.zeros(2, 3, 2, 1)], idx)
    with pytest.raises(ValueError, match="r_0 must be 1"):
        ops.ttm_gather_fits([3], [2], [2, 1])
    with pytest.raises(ValueError, match="r_0 must be 1"):
        ops.ttm_gather_fits([2] * 5, [2] * 5, [2, 2, 2, 2, 2, 1])
    with pytest.raises(ValueError, match="left rank"):
        HF.ttm_embedding([torch.zeros(1, 3, 2, 4), torch.zeros(5, 3, 2, 1)], idx)
    with pytest.raises(ValueError, match="at most 4 modes"):
        ops.ttm_gather([torch.zeros(1, 2, 2, 1)] * 5, idx)
    with pytest.raises(ValueError, match="at most 4 modes"):
        ops.ttm_gather_plan([2] * 5, [2] * 5, [1] * 6)
    for bad in (torch.zeros(3), torch.zeros(3, dtype=torch.bool), torch.zeros(3, dtype=torch.float64)):
        with pytest.raises(TypeError, match="integer"):
            HF.ttm_embedding([torch.zeros(1, 3, 2, 1)], bad)
    with pytest.raises(TypeError, match="int32 or int64"):
        ops.ttm_gather([torch.zeros(1, 3, 2, 1)], torch.zeros(3))
    # the checks above ran before any device was touched; what is left needs one
    with pytest.raises(_cabi.TadmmError, match="no CPU"):
        HF.ttm_embedding([torch.zeros(1, 3, 2, 1)], idx)


@pytest.mark.parametrize("name", [k for k in R.SHAPES])
def test_float32_restatement_is_within_2e6_of_float64(name):
    """What float32 arithmetic costs at the shapes and token sets of the GPU tests: the bar of those tests (1e-5) sits
    well above it.  Measured: output <= 4.2e-7, gradients <= 5.1e-7 with up to 130 duplicates of one token."""
    shape = R.SHAPES[name]
    cores = R.make_cores(shape)
    tile = ops.ttm_gather_plan(*shape)[2]
    for ts in R.TOKEN_SETS:
        idx = R.token_set(ts, shape, tile)
        y64, y32 = R.forward(cores, idx), R.forward(cores, idx, np.float32)
        assert y32.dtype == np.float32 and R.rel_err(y32, y64) < 2e-6, (ts, R.rel_err(y32, y64))
        dy = np.random.default_rng(5).standard_normal(y64.shape).astype(np.float32)
        for g32, g64 in zip(R.backward(cores, idx, dy, np.float32), R.backward(cores, idx, dy)):
            assert R.rel_err(g32, g64) < 2e-6, (ts, R.rel_err(g32, g64))
