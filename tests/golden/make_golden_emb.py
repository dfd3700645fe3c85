"""Generate golden vectors G10 (the factorised embeddings) from the REAL reference.

    python tests/golden/make_golden_emb.py <path of the reference checkout>

Runs only where the reference is at hand: imports its xcompression/transformer/{TTEmbedding,TTMEmbedding,SVDEmbedding}.py
and records state_dicts, index tensors and forward outputs (CPU, fixed seed), the rank helpers at a handful of shapes,
the table `init_pretrained_emb` reconstructs and the product of the factors `SVDEmbedding(weights=)` makes, as small
.npz / .json fixtures.  The reference never travels with the tests; these data files do.

tensorly is not needed for more than one call, so a stand-in module serves: a no-op `set_backend` and a `tt_to_tensor`
that multiplies the factors (r, n, r') left to right and drops the two boundary ranks of 1.

The pretrained tables have an exact low-rank part plus noise four orders of magnitude below it, so the truncated
decompositions are well conditioned and their reconstructions unique at fp32 precision (singular-vector signs are
not, which is why reconstructions and not cores are recorded).
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True


def _tt_to_tensor(factors):
    full = factors[0].reshape(-1, factors[0].shape[-1])
    shape = [factors[0].shape[1]]
    for f in factors[1:]:
        full = full.reshape(-1, f.shape[0]) @ f.reshape(f.shape[0], -1)
        shape.append(f.shape[1])
    return full.reshape(shape)


def load_reference(path):
    tl = types.ModuleType("tensorly")
    tl.set_backend = lambda name: None
    tl.tt_to_tensor = _tt_to_tensor
    sys.modules["tensorly"] = tl
    sys.path.insert(0, os.path.join(path, "xcompression", "transformer"))
    import SVDEmbedding as svd_mod
    import TTEmbedding as tt_mod
    import TTMEmbedding as ttm_mod
    return tt_mod, ttm_mod, svd_mod


TTM_CASES = {
    "ttm_d2": ([3, 2], [2, 3], [1, 5, 1]),
    "ttm_d3": ([4, 3, 5], [3, 1, 5], [1, 17, 33, 1]),
    "ttm_d4": ([3, 2, 2, 3], [2, 1, 3, 2], [1, 4, 6, 5, 1]),
}
TT_CASES = {
    "tt_3in_2out": ([5, 7, 3], [4, 6], [1, 16, 20, 24, 5, 1]),
    "tt_2in_3out": ([4, 6], [2, 3, 2], [1, 4, 9, 6, 2, 1]),
}
SVD_CASES = {"svd_7x12_r33": (7, 12, 33), "svd_50x20_r6": (50, 20, 6)}
RANKS_TT = [([13, 13, 13, 14, 8, 4, 4, 6], 5), ([50, 52, 55, 2, 2, 4], 3), ([30522, 768], 5), ([32, 31, 31, 12, 8, 8], 10),
            ([200, 220, 250, 4, 4, 8], 20)]
RANKS_TTM = [([32, 31, 31], [12, 8, 8], 5), ([32, 31, 31], [12, 8, 8], 20), ([200, 220, 250], [4, 4, 8], 10),
             ([10, 10, 10, 10], [4, 4, 4, 4], 8)]


def indices(rng, total, shape):
    idx = rng.integers(0, total, size=shape)
    idx.reshape(-1)[0], idx.reshape(-1)[-1] = 0, total - 1
    return idx.astype(np.int64)


def record(out, meta, key, layer, idx, **info):
    with torch.no_grad():
        y = layer(torch.from_numpy(idx)).contiguous().numpy()
    out[key + "_index"], out[key + "_y"] = idx, y
    names = []
    for n, t in layer.state_dict().items():
        names.append([n, list(t.shape)])
        out[f"{key}_sd_{n}"] = t.detach().numpy()
    meta["cases"][key] = dict(state_dict=names, **info)


def low_tt_table(rng, shapes, ranks, noise):
    full = _tt_to_tensor([torch.from_numpy(rng.standard_normal((ranks[i], shapes[i], ranks[i + 1])))
                          for i in range(len(shapes))]).numpy()
    full = full / np.abs(full).max()
    return (full + noise * rng.standard_normal(full.shape)).astype(np.float32)


def main():
    tt_mod, ttm_mod, svd_mod = load_reference(sys.argv[1])
    rng = np.random.default_rng(20220211)
    torch.manual_seed(0)
    out, meta = {}, {"cases": {}, "ranks_tt": [], "ranks_ttm": []}
    for key, (n, m, r) in TTM_CASES.items():
        layer = ttm_mod.TTMEmbedding(n, m, r)
        record(out, meta, key, layer, indices(rng, int(np.prod(n)), (3, 5)), cls="TTM", input_tt_shape=n,
               output_tt_shape=m, tt_ranks=r)
    for key, (n, m, r) in TT_CASES.items():
        layer = tt_mod.TTEmbedding(n, m, tt_ranks=r)
        record(out, meta, key, layer, indices(rng, int(np.prod(n)), (2, 7)), cls="TT", input_tt_shape=n,
               output_tt_shape=m, tt_ranks=r)
    for key, (rows, dim, rank) in SVD_CASES.items():
        layer = svd_mod.SVDEmbedding(rows, dim, rank=rank)
        record(out, meta, key, layer, indices(rng, rows, (4, 3)), cls="SVD", num_embeddings=rows, embedding_dim=dim,
               rank=rank)
    for shapes, ratio in RANKS_TT:
        meta["ranks_tt"].append(dict(tt_shapes=shapes, ratio=ratio,
                                     ranks=[int(v) for v in tt_mod.compute_ranks_tt(shapes, ratio)]))
    for n, m, ratio in RANKS_TTM:
        layer = ttm_mod.TTMEmbedding(n, m, [1] * (len(n) + 1))
        meta["ranks_ttm"].append(dict(input_tt_shape=n, output_tt_shape=m, ratio=ratio,
                                      ranks=[int(v) for v in layer.compute_ranks_ttm(ratio)]))
    # init_pretrained_emb: 60 x 24 table, exact sizes, TT ranks (1, 3, 6, 8, 4, 1) plus noise; kept at those ranks
    n, m, r = [3, 4, 5], [4, 6], [1, 3, 6, 8, 4, 1]
    table = low_tt_table(rng, n + m, r, 1e-4).reshape(60, 24)
    layer = tt_mod.TTEmbedding(n, m, tt_ranks=list(r))
    layer.init_pretrained_emb(torch.from_numpy(table))
    out["pretrained_table"] = table
    out["pretrained_recon"] = layer.tt2ten().numpy().reshape(60, 24).astype(np.float32)
    meta["pretrained"] = dict(input_tt_shape=n, output_tt_shape=m, tt_ranks=r)
    # SVDEmbedding(weights=): 40 x 24, rank 6 plus noise
    u, v = rng.standard_normal((40, 6)), rng.standard_normal((6, 24))
    w = u @ v
    w = (w / np.abs(w).max() + 1e-4 * rng.standard_normal(w.shape)).astype(np.float32)
    layer = svd_mod.SVDEmbedding(40, 24, rank=6, weights=torch.from_numpy(w))
    out["svd_weights"] = w
    out["svd_recon"] = (layer.first_factor.detach() @ layer.last_factor.detach()).numpy().astype(np.float32)
    meta["svd_weights"] = dict(num_embeddings=40, embedding_dim=24, rank=6,
                               state_dict=[[k, list(t.shape)] for k, t in layer.state_dict().items()])
    np.savez_compressed(os.path.join(HERE, "g10_embeddings.npz"), **out)
    json.dump(meta, open(os.path.join(HERE, "g10_embeddings.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
