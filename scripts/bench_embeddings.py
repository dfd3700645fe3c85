"""The factorised embeddings (TTMEmbedding, TTEmbedding, SVDEmbedding) at BERT-sized tables, 512 and 4096 tokens,
forward (inference) and forward + backward.

Paths:  native   -- the layer on the launches, whatever `ops.ttm_gather_pays` says: one tadmm_ttm_gather_fwd launch (+
                    the dense product of TT / SVD); backward one tadmm_ttm_gather_bwd launch per core
        composed -- the same layer with the lookup forced down the composed device route (div / fmod / slice selection /
                    bmm under autograd: functional.ttm_embedding_composed), the reference's own steps
        dense    -- F.embedding on a dense table of the same size (what the factorisation replaces)
Timing: HIP events around a window of about 250 ms of calls after a warm-up of every path, 7 rounds with the order of
the paths rotated every round; the median and the spread (min..max) of the rounds are reported, in microseconds per
call.
`gflops` (native forward): the multiply-adds of the gather chain, 2 * tokens * sum_k P_{k-1} r_{k-1} m_k r_k, over the
time of the whole forward call.

    python scripts/bench_embeddings.py [--quick] [--json OUT]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "dnn-compression-tensor-admm_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tadmm import emb_layers, ops  # noqa: E402

DEV = torch.device("cuda", 0)
TOKENS = (512, 4096)


def layers():
    return [
        ("TTMEmbedding [32,31,31]->[12,8,8] r57", 32 * 31 * 31, 768,
         lambda: emb_layers.TTMEmbedding([32, 31, 31], [12, 8, 8], [1, 57, 57, 1])),
        ("TTEmbedding [13,13,13,14]->[8,4,4,6] ratio 5", 13 * 13 * 13 * 14, 768,
         lambda: emb_layers.TTEmbedding([13, 13, 13, 14], [8, 4, 4, 6], compression_ratio=5)),
        ("SVDEmbedding 30522x768 r128", 30522, 768, lambda: emb_layers.SVDEmbedding(30522, 768, rank=128)),
    ]


def gather_flops(layer, tokens):
    if isinstance(layer, emb_layers.SVDEmbedding):
        return 0.0
    cores = list(layer.cores)
    if isinstance(layer, emb_layers.TTEmbedding):
        cores = [c.unsqueeze(2) for c in cores[:len(layer.input_tt_shape)]]
    P, f = 1, 0
    for c in cores:
        f += P * c.shape[0] * c.shape[2] * c.shape[3]
        P *= c.shape[2]
    return 2.0 * tokens * f


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters          # microseconds per call


def make_paths(layer, table, idx, train):
    params = list(layer.parameters())

    def run(mod_forward):
        if not train:
            with torch.no_grad():
                return mod_forward()
        y = mod_forward()
        for p in params:
            p.grad = None
        y.backward(grad)
        return y

    def forced(pays):
        keep = ops.ttm_gather_pays
        ops.ttm_gather_pays = lambda *a, **k: pays      # both routes are measured whatever the shipped rule says
        try:
            return run(lambda: layer(idx))
        finally:
            ops.ttm_gather_pays = keep

    def native():
        return forced(True)

    def composed():
        return forced(False)

    def dense():
        if not train:
            with torch.no_grad():
                return F.embedding(idx, table)
        table.grad = None
        y = F.embedding(idx, table)
        y.backward(grad)
        return y

    with torch.no_grad():
        grad = torch.randn_like(layer(idx))
    return {"native": native, "composed": composed, "dense": dense}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_embeddings.py measures on the GPU; no device found")
    rounds = 3 if args.quick else 7
    window_us = 3.0e4 if args.quick else 2.5e5       # a timed window: 250 ms of calls (30 ms with --quick)
    results = []
    for label, rows, dim, make in layers():
        torch.manual_seed(0)
        layer = make().to(DEV)
        table = torch.randn(rows, dim, device=DEV, requires_grad=True)
        for tokens in TOKENS:
            idx = torch.randint(0, rows, (tokens,), device=DEV)
            for train in (False, True):
                paths = make_paths(layer, table, idx, train)
                check = make_paths(layer, table, idx, False)
                a, b = check["native"](), check["composed"]()
                diff = float((a - b).abs().max()) / float(b.abs().max())
                iters = {}
                for name, fn in paths.items():           # warm-up of every path, and the length of its window
                    for _ in range(3):
                        fn()
                    t = window(fn, 5)
                    iters[name] = int(min(20000, max(10, window_us / max(t, 1.0))))
                times = {name: [] for name in paths}
                order = list(paths)
                for r in range(rounds):
                    for name in order[r % 3:] + order[:r % 3]:
                        times[name].append(window(paths[name], iters[name]))
                row = dict(layer=label, tokens=tokens, mode="fwd+bwd" if train else "fwd", native_vs_composed=diff)
                for name, ts in times.items():
                    row[name] = dict(median=statistics.median(ts), min=min(ts), max=max(ts), iters=iters[name])
                if not train and gather_flops(layer, tokens):
                    row["gflops"] = gather_flops(layer, tokens) / row["native"]["median"] * 1e-3
                results.append(row)
                print(json.dumps(row), flush=True)
    print("\n| layer | tokens | mode | native us | composed us | dense us | composed / native |")
    print("|---|---|---|---|---|---|---|")
    for r in results:
        cell = lambda k: f"{r[k]['median']:.1f} ({r[k]['min']:.1f}..{r[k]['max']:.1f})"  # noqa: E731
        print(f"| {r['layer']} | {r['tokens']} | {r['mode']} | {cell('native')} | {cell('composed')} | {cell('dense')} "
              f"| {r['composed']['median'] / r['native']['median']:.2f} |")
    if args.json:
        json.dump(results, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
