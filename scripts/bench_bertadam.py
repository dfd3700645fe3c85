"""BertAdam step: the two-launch native route (csrc/bertadam.hip) against what else can take the step.

    python scripts/bench_bertadam.py [--repeats 7] [--budget 0.15] [--workloads tt_encoder tt_bert dense_bert]

Workloads are tables of tensor shapes, re-derived from the reference's model code (no model is built):
    tt_encoder   the 12 encoder layers of the BERT-base that xcompression/transformer/compressed_modeling_tt.py builds:
                 per layer four attention maps of three TT cores each (768 x [24, 32], ranks 18), the intermediate map
                 (768 -> [64, 48], ranks 18), the output map ([48, 64] -> 768, ranks 17) and two LayerNorms; TTLinear is
                 constructed without a bias there.  264 tensors, most of them a few thousand elements.
    tt_bert      tt_encoder plus what stays dense in that model: word (30522 x 768), position and token-type embeddings,
                 their LayerNorm, the pooler and a two-class head.  273 tensors; the word embedding is 91 % of the bytes.
    dense_bert   BERT-base with dense linear layers, the large-tensor case.  201 tensors, 109 M elements.

Routes, all on the same float32 tensors with max_grad_norm = 1 and weight_decay = 0.01:
    native       `ops.BertAdamPlan.step`: two launches for the whole list
    optimizer    `tadmm.optimization.BertAdam.step()` around it (gradients already in the plan's buffer: nothing staged)
    foreach      `ops.bert_adam_composed`: the same arithmetic on torch._foreach_* calls
    loop         the reference's per-tensor loop restated (norm, clip in place, the moment updates, the update, one
                 tensor after the other: about twenty launches per tensor)
    adamw_fused  `torch.optim.AdamW(fused=True)`: DIFFERENT arithmetic (bias correction, no clipping); a bandwidth marker

Every figure: median of `--repeats` windows, host clock around work that ends in a device synchronise, after 3 warm-up
calls; a window holds as many calls as fit `--budget` seconds (3 .. 200); min..max of the windows is the spread.
`GB/s` counts 8 x 4 x numel bytes per step (g read by the norm launch; p, g, m, v read and p, m, v written by the update).
`ahead` names the route whose max is below the other's min (native against foreach), else 'level'.

Measured on an MI355X:
    (ms per step, median (min..max); native also in bytes per second)
    workload    native                               optimizer             foreach            loop               adamw_fused
    tt_encoder  0.0285 (0.0279..0.0287)  2.03 TB/s   0.212 (0.209..0.213)  2.34 (2.34..2.72)  18.9 (18.5..19.0)  0.388 (0.374..0.391)
    tt_bert     0.154  (0.154..0.156)    5.45 TB/s   0.220 (0.217..0.220)  2.45 (2.44..5.15)  19.2 (19.0..19.4)  0.387 (0.386..0.389)
    dense_bert  0.664  (0.663..0.664)    5.28 TB/s   0.657 (0.657..0.659)  3.14 (3.14..3.15)  14.2 (14.1..14.3)  0.682 (0.682..0.684)
    native is ahead of foreach on all three (82x, 15.9x, 4.7x): there is no routing rule.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dnn-compression-tensor-admm_amd"))

from tadmm import ops  # noqa: E402
from tadmm.optimization import BertAdam  # noqa: E402

DEV = "cuda:0"
HIDDEN, LAYERS, INTER, VOCAB, POSITIONS, TYPES, LABELS = 768, 12, 3072, 30522, 512, 2, 2
HYPER = dict(b1=0.9, b2=0.999, e=1e-6, weight_decay=0.01, max_grad_norm=1.0)
LR = 1e-4


def tt_cores(shapes, ranks):
    return [(ranks[i], shapes[i], ranks[i + 1]) for i in range(len(shapes))]


def layer_norm():
    return [(HIDDEN,), (HIDDEN,)]


def tt_encoder_shapes():
    out = []
    for _ in range(LAYERS):
        for _ in range(4):                                             # query, key, value, attention output
            out += tt_cores([HIDDEN, 24, 32], [1, 18, 18, 1])
        out += layer_norm()
        out += tt_cores([64, 48, HIDDEN], [1, 18, 18, 1])              # intermediate: out_shapes + in_shapes
        out += tt_cores([HIDDEN, 48, 64], [1, 17, 17, 1])              # output
        out += layer_norm()
    return out


def dense_rest_shapes():
    return [(VOCAB, HIDDEN), (POSITIONS, HIDDEN), (TYPES, HIDDEN)] + layer_norm() + \
           [(HIDDEN, HIDDEN), (HIDDEN,), (LABELS, HIDDEN), (LABELS,)]


def dense_bert_shapes():
    out = []
    for _ in range(LAYERS):
        for _ in range(4):
            out += [(HIDDEN, HIDDEN), (HIDDEN,)]
        out += layer_norm()
        out += [(INTER, HIDDEN), (INTER,), (HIDDEN, INTER), (HIDDEN,)]
        out += layer_norm()
    return out + dense_rest_shapes()


WORKLOADS = {
    "tt_encoder": tt_encoder_shapes,
    "tt_bert": lambda: tt_encoder_shapes() + dense_rest_shapes(),
    "dense_bert": dense_bert_shapes,
}


def windows(fn, repeats, budget):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    iters = max(3, min(200, int(budget / max(time.perf_counter() - t0, 1e-6))))
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters * 1e3)
    return out, iters


def reference_loop(ps, gs, ms, vs, lr, b1, b2, e, weight_decay, max_grad_norm):
    for p, g, m, v in zip(ps, gs, ms, vs):
        if max_grad_norm > 0:
            g.mul_(torch.clamp(max_grad_norm / (torch.linalg.vector_norm(g) + 1e-6), max=1.0))
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        update = m / (v.sqrt() + e)
        if weight_decay > 0:
            update += weight_decay * p
        p.add_(-(lr * update))


def tensors(shapes, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ps = [0.05 * torch.randn(s, device=DEV, generator=g) for s in shapes]
    gs = [0.01 * torch.randn(s, device=DEV, generator=g) for s in shapes]
    return ps, gs, [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]


def routes(shapes):
    def native():
        ps, gs, ms, vs = tensors(shapes, 1)
        plan = ops.BertAdamPlan(list(zip(ps, gs, ms, vs)))
        return lambda: plan.step(LR, **HYPER)

    def optimizer():
        ps, gs, _, _ = tensors(shapes, 1)
        params = [torch.nn.Parameter(p) for p in ps]
        opt = BertAdam(params, lr=LR, schedule="none", **HYPER)
        for p, g in zip(params, gs):
            p.grad = g
        opt.step()                                   # builds the plan and stages once; .grad now points into it
        return opt.step

    def foreach():
        ps, gs, ms, vs = tensors(shapes, 1)
        return lambda: ops.bert_adam_composed(ps, gs, ms, vs, LR, **HYPER)

    def loop():
        ps, gs, ms, vs = tensors(shapes, 1)
        return lambda: reference_loop(ps, gs, ms, vs, LR, **HYPER)

    def adamw_fused():
        ps, gs, _, _ = tensors(shapes, 1)
        params = [torch.nn.Parameter(p) for p in ps]
        for p, g in zip(params, gs):
            p.grad = g
        return torch.optim.AdamW(params, lr=LR, weight_decay=0.01, fused=True).step

    return [("native", native), ("optimizer", optimizer), ("foreach", foreach), ("loop", loop),
            ("adamw_fused", adamw_fused)]


def agreement(shapes):
    """The native and the foreach route must compute the same thing at the sizes timed: worst max|a-b| / max|b| of p."""
    a, b = tensors(shapes, 2), tensors(shapes, 2)
    ops.BertAdamPlan(list(zip(*a))).step(1e-2, **HYPER)
    ops.bert_adam_composed(*b, 1e-2, **HYPER)
    return max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(a[0], b[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--budget", type=float, default=0.15)
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bertadam.py needs the MI355X: a timing taken elsewhere says nothing")
    for name in a.workloads:
        shapes = WORKLOADS[name]()
        numel = sum(int(torch.Size(s).numel()) for s in shapes)
        row = {"workload": name, "tensors": len(shapes), "numel": numel, "rel_diff": agreement(shapes)}
        for route, make in routes(shapes):
            ws, iters = windows(make(), a.repeats, a.budget)
            med = statistics.median(ws)
            row[route] = {"median_ms": med, "min_ms": min(ws), "max_ms": max(ws), "iters": iters,
                          "GBps": 32.0 * numel / (med * 1e-3) / 1e9}
            torch.cuda.empty_cache()
        n, f = row["native"], row["foreach"]
        row["ahead"] = "native" if n["max_ms"] < f["min_ms"] else "foreach" if f["max_ms"] < n["min_ms"] else "level"
        row["speedup_vs_foreach"] = f["median_ms"] / n["median_ms"]
        row["speedup_vs_loop"] = row["loop"]["median_ms"] / n["median_ms"]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
