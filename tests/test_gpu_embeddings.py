"""The gathered TT-matrix chain (csrc/ttm_gather.hip) and the three embedding layers on the MI355X, against the float64
restatement of tests/_emb_ref.py and the reference's recorded outputs.  Error measure: max|a - ref| / max|ref|, bar 1e-5
(float32 arithmetic itself stays under 2e-6 at these shapes: tests/test_embeddings_host_cpu.py)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import _emb_ref as R
from tadmm import emb_layers, ops
from tadmm import functional as HF

pytestmark = pytest.mark.gpu
BAR = 1e-5
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def reference(name, ts):
    """(index array, float64 output, dy, float64 gradients) of one case, computed once."""
    shape = R.SHAPES[name]
    cores = R.make_cores(shape)
    idx = R.token_set(ts, shape, ops.ttm_gather_plan(*shape)[2])
    if ts == "transposed":
        idx = np.ascontiguousarray(idx.T)            # the values the transposed view shows, in its own order
    y = R.forward(cores, idx)
    dy = np.random.default_rng(5).standard_normal(y.shape).astype(np.float32)
    return idx, y, dy, R.backward(cores, idx, dy)


def device_cores(name):
    return [torch.from_numpy(c).to(DEV).requires_grad_(True) for c in R.make_cores(R.SHAPES[name])]


def device_index(ts, idx):
    dtype = torch.int32 if ts in ("random130", "transposed") else torch.int64
    if ts == "transposed":
        t = torch.from_numpy(np.ascontiguousarray(idx.T)).to(DEV, dtype).t()     # a (7, 5) view of a (5, 7) buffer
        assert not t.is_contiguous()
        return t
    return torch.from_numpy(idx).to(DEV, dtype)


@pytest.mark.parametrize("ts", R.TOKEN_SETS)
@pytest.mark.parametrize("name", list(R.SHAPES))
def test_forward_and_gradients(name, ts):
    n, m, r = R.SHAPES[name]
    idx_np, y_ref, dy_np, g_ref = reference(name, ts)
    cores = device_cores(name)
    idx = device_index(ts, idx_np)
    fits = ops.ttm_gather_fits(n, m, r)
    assert fits == (name != "lds_past")
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    dy = torch.from_numpy(dy_np).to(DEV)
    runs = []
    for _ in range(2):
        for c in cores:
            c.grad = None
        y = HF.ttm_embedding(cores, idx, counter, route="native" if fits else None)
        assert y.shape == tuple(idx.shape) + (y_ref.shape[1],) and y.dtype == torch.float32
        y.reshape(dy.shape).backward(dy)
        runs.append([c.grad.clone() for c in cores])
    err = R.rel_err(y.detach().reshape(y_ref.shape).cpu().numpy(), y_ref)
    print(f"{name}/{ts}: output {err:.2e}")
    assert err < BAR
    ik = R.split_index(idx_np, n)
    for k, (g1, g2, gr) in enumerate(zip(runs[0], runs[1], g_ref)):
        e = R.rel_err(g1.cpu().numpy(), gr)
        print(f"{name}/{ts}: core {k} gradient {e:.2e}")
        assert e < BAR
        assert torch.equal(g1, g2), "gradients differ between two calls"
        unused = sorted(set(range(n[k])) - set(ik[:, k].tolist()))
        if unused:
            assert torch.count_nonzero(g1[:, unused]).item() == 0, "a slice no token selects is not exactly zero"
    assert int(counter.item()) == 0
    if fits:
        flat = idx.reshape(-1)
        out = torch.full(y_ref.shape, float("nan"), device=DEV)
        ops.ttm_gather([c.detach() for c in cores], flat, out=out)
        assert torch.equal(out, y.detach().reshape(out.shape)), "a row of the poisoned buffer was not written"


@pytest.mark.parametrize("name", ["svd_row", "d3", "d4", "lds_past"])
def test_bad_indices_give_zero_rows_and_are_counted(name):
    """Bad input, handled: the bounds check of the kernel (and of the composed route) is what is under test."""
    n, m, r = R.SHAPES[name]
    total = int(np.prod(n))
    idx_np = R.token_set("ends", R.SHAPES[name], 1).copy()
    idx_np[1], idx_np[7] = -1, total
    cores = device_cores(name)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    route = "native" if ops.ttm_gather_fits(n, m, r) else None
    y = HF.ttm_embedding(cores, torch.from_numpy(idx_np).to(DEV), counter, route=route)
    y_ref = R.forward(R.make_cores(R.SHAPES[name]), idx_np)
    dy_np = np.random.default_rng(5).standard_normal(y_ref.shape).astype(np.float32)
    y.backward(torch.from_numpy(dy_np).to(DEV))
    torch.cuda.synchronize()
    assert int(counter.item()) == 2
    out = y.detach().cpu().numpy()
    assert not out[1].any() and not out[7].any() and not y_ref[1].any()
    assert R.rel_err(out, y_ref) < BAR
    for c, gr in zip(cores, R.backward(R.make_cores(R.SHAPES[name]), idx_np, dy_np)):
        assert R.rel_err(c.grad.cpu().numpy(), gr) < BAR


@pytest.fixture(scope="module")
def golden(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, "g10_embeddings.json")))
    return meta, np.load(os.path.join(golden_dir, "g10_embeddings.npz"))


def _layer_of(c):
    if c["cls"] == "TTM":
        return emb_layers.TTMEmbedding(c["input_tt_shape"], c["output_tt_shape"], c["tt_ranks"])
    if c["cls"] == "TT":
        return emb_layers.TTEmbedding(c["input_tt_shape"], c["output_tt_shape"], tt_ranks=c["tt_ranks"])
    return emb_layers.SVDEmbedding(c["num_embeddings"], c["embedding_dim"], rank=c["rank"])


def test_modules_load_reference_state_dicts_and_match(golden):
    meta, data = golden
    assert len(meta["cases"]) == 7
    for key, c in meta["cases"].items():
        layer = _layer_of(c)
        sd = {k: torch.from_numpy(data[f"{key}_sd_{k}"]) for k, _ in c["state_dict"]}
        assert list(layer.state_dict().keys()) == list(sd.keys())
        layer.load_state_dict(sd, strict=True)
        layer = layer.to(DEV)
        idx = torch.from_numpy(data[key + "_index"]).to(DEV)
        ref = data[key + "_y"]            # (the reference's TTMEmbedding returns its rows flat: (tokens, size))
        # with gradients `ops.ttm_gather_pays` may send the lookup down the composed route; without, it is the launch
        with torch.no_grad():
            outs = {"inference": layer(idx)}
        outs["training"] = layer(idx)
        assert outs["inference"].grad_fn is None and outs["training"].grad_fn is not None
        for mode, y in outs.items():
            assert y.shape == tuple(idx.shape) + (ref.shape[-1],) and y.numel() == ref.size
            err = R.rel_err(y.detach().cpu().numpy().reshape(ref.shape), ref)
            print(f"{key} ({mode}): {err:.2e}")
            assert err < BAR
        assert int(layer.bad_index_count.item()) == 0


def _composed_f64(layer, idx):
    """The layer as torch ops in float64 on copies of its parameters; returns (output, parameters)."""
    ps = [p.detach().double().requires_grad_(True) for p in layer.parameters()]
    if isinstance(layer, emb_layers.SVDEmbedding):
        rows = HF.ttm_embedding_composed([ps[0].reshape(1, ps[0].shape[0], 1, -1)], idx)
        return rows @ ps[1], ps
    din = len(layer.input_tt_shape)
    rows = HF.ttm_embedding_composed([p.unsqueeze(2) for p in ps[:din]], idx)
    tail = ps[din].reshape(ps[din].shape[0], -1)
    for p in ps[din + 1:]:
        tail = tail.reshape(-1, p.shape[0]) @ p.reshape(p.shape[0], -1)
    return rows @ tail.reshape(rows.shape[-1], -1), ps


@pytest.mark.parametrize("tokens", [(6, 11), (40, 30)])        # either side of ops.TTM_GRAD_MAX_TOKENS: both routes
@pytest.mark.parametrize("which", ["svd", "tt"])
def test_layer_backward_matches_float64_autograd(which, tokens):
    torch.manual_seed(3)
    if which == "svd":
        layer = emb_layers.SVDEmbedding(50, 20, rank=6).to(DEV)
        total = 50
    else:
        layer = emb_layers.TTEmbedding([5, 7, 3], [4, 6], tt_ranks=[1, 16, 20, 24, 5, 1]).to(DEV)
        total = 105
    idx = torch.randint(0, total, tokens, device=DEV)
    y = layer(idx)
    w = torch.randn_like(y)
    (y * w).sum().backward()
    y64, ps = _composed_f64(layer, idx)
    (y64 * w.double()).sum().backward()
    assert R.rel_err(y.detach().cpu().numpy(), y64.detach().cpu().numpy()) < BAR
    with torch.no_grad():                                  # the inference route of the same layer
        assert R.rel_err(layer(idx).cpu().numpy(), y64.detach().cpu().numpy()) < BAR
    for p, p64 in zip(layer.parameters(), ps):
        assert R.rel_err(p.grad.cpu().numpy(), p64.grad.cpu().numpy()) < BAR


def test_pretrained_initialisers_match_reference(golden):
    meta, data = golden
    p = meta["pretrained"]
    layer = emb_layers.TTEmbedding(p["input_tt_shape"], p["output_tt_shape"], tt_ranks=list(p["tt_ranks"])).to(DEV)
    layer.init_pretrained_emb(torch.from_numpy(data["pretrained_table"]))
    assert R.rel_err(layer.tt2ten().reshape(60, 24).cpu().numpy(), data["pretrained_recon"]) < BAR
    assert R.rel_err(layer.restore_weights().detach().cpu().numpy(), data["pretrained_recon"]) < BAR
    idx = torch.arange(60, device=DEV)
    assert R.rel_err(layer(idx).detach().cpu().numpy(), data["pretrained_recon"]) < BAR
    with torch.no_grad():                                  # the launch (inference) as well as the training route
        assert R.rel_err(layer(idx).cpu().numpy(), data["pretrained_recon"]) < BAR
    # a shorter table is zero-padded (the stated deviation).  At full TT ranks the decomposition is exact, so the rows
    # that exist come back and the padding is zero, both to the float32 bar
    full_ranks = [1, 3, 12, 24, 6, 1]
    layer = emb_layers.TTEmbedding(p["input_tt_shape"], p["output_tt_shape"], tt_ranks=full_ranks).to(DEV)
    layer.init_pretrained_emb(torch.from_numpy(data["pretrained_table"][:48]))
    padded = np.concatenate([data["pretrained_table"][:48], np.zeros((12, 24), np.float32)])
    assert R.rel_err(layer.restore_weights().detach().cpu().numpy(), padded) < BAR
    s = meta["svd_weights"]
    layer = emb_layers.SVDEmbedding(s["num_embeddings"], s["embedding_dim"], rank=s["rank"],
                                    weights=torch.from_numpy(data["svd_weights"]))
    assert [[k, list(v.shape)] for k, v in layer.state_dict().items()] == s["state_dict"]
    layer = layer.to(DEV)
    recon = (layer.first_factor @ layer.last_factor).detach().cpu().numpy()
    assert R.rel_err(recon, data["svd_recon"]) < BAR


def test_steady_state_forward_allocates_only_the_output():
    n, m, r = R.SHAPES["bert_ttm"]
    layer = emb_layers.TTMEmbedding(n, m, r).to(DEV)
    idx = torch.randint(0, int(np.prod(n)), (4, 64), device=DEV)
    with torch.no_grad():
        layer(idx)                                        # first call: handle, code object, LDS attribute
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        y = layer(idx)
    torch.cuda.synchronize()
    out_bytes = -(-y.numel() * 4 // 512) * 512            # the caching allocator hands out multiples of 512 bytes
    assert torch.cuda.memory_allocated() - before == out_bytes
    assert torch.cuda.max_memory_allocated() - before == out_bytes, "a temporary lived during the forward"
    assert y.shape == (4, 64, 768) and int(layer.bad_index_count.item()) == 0
    ref = HF.ttm_embedding_composed([c.detach().double() for c in layer.cores], idx)
    assert R.rel_err(y.cpu().numpy(), ref.cpu().numpy()) < BAR
