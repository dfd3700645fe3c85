"""The dropout + residual + LayerNorm tail of a BERT sub-layer, and a whole BertLayer: the launch (csrc/bertnorm.hip)
against the composed torch route (`functional.residual_layer_norm_composed`: F.dropout, the add, F.layer_norm) and
against the reference's literal ten-call BertLayerNorm behind F.dropout and the add (compressed_modeling_tt.py:145-158,
:437-438 -- what a user of the reference comes from; restated here).

    python scripts/bench_bertlayer.py [--repeats 5] [--window-ms 50] [--quick] [--skip-layer]

Tail classes: rows = B * S for B in {1, 8, 32} and S in {64, 128, 512}, hidden in {312, 768, 1024}, float32 and bfloat16
(parameters in the type of x on every route), a forward in eval mode under no_grad and a training step (dropout 0.1 drawn
by each route's own torch call, gradients into x, res, weight and bias).  For the largest class the bytes the launch has
to move (forward: x, res, y; step: also keep twice, g, dx, dres) over its time stand next to the 6.29 TB/s copy rate.

Layer classes: BertLayer(768, 12 heads, 3072) with the reference's TT shapes, float32, S = 128, B in {1, 8, 32}: every
piece routed by its measured rule (`route=None`) against every piece composed, forward and training step.

Every figure: median of `--repeats` windows, host clock around work that ends in a device synchronise, after 3 warm-up
calls per class and route; a window holds as many calls as fill `--window-ms` (3 to 200, fixed from one timed call);
min..max of the windows is the spread.  `ahead` names a route only when its max is below the other's min, the rule every
`*_pays` function follows; otherwise it says `level`.  One JSON line per class."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dnn-compression-tensor-admm_amd"))

from tadmm import bert_layers as BL  # noqa: E402
from tadmm import functional as HF  # noqa: E402

DEV = "cuda:0"
BATCHES = (1, 8, 32)
LENGTHS = (64, 128, 512)
WIDTHS = (312, 768, 1024)
COPY_TBS = 6.29
P = 0.1


def windows(fn, repeats, window_ms):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    iters = max(3, min(200, int(window_ms * 1e-3 / max(time.perf_counter() - t0, 1e-6))))
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters * 1e3)
    return out, iters


def summary(ws, iters):
    return {"median_ms": statistics.median(ws), "min_ms": min(ws), "max_ms": max(ws), "iters": iters}


def verdict(a, b, names):
    """names[0] / names[1] when one is ahead beyond the spread of both, else 'level'."""
    if a["max_ms"] < b["min_ms"]:
        return names[0]
    if b["max_ms"] < a["min_ms"]:
        return names[1]
    return "level"


def literal(x, res, weight, bias, p, training):
    """The reference's own string of calls: nn.Dropout, the add, then BertLayerNorm.forward."""
    h = F.dropout(x, p, training) + res
    u = h.mean(-1, keepdim=True)
    s = (h - u).pow(2).mean(-1, keepdim=True)
    h = (h - u) / torch.sqrt(s + 1e-12)
    return weight * h + bias


def tail(B, S, hidden, dtype, what, repeats, window_ms):
    g = torch.Generator(device=DEV).manual_seed(B * 4099 + S + hidden)
    x, res = (torch.randn(B, S, hidden, device=DEV, generator=g).to(dtype) for _ in range(2))
    weight = (1 + 0.1 * torch.randn(hidden, device=DEV, generator=g)).to(dtype)
    bias = (0.1 * torch.randn(hidden, device=DEV, generator=g)).to(dtype)
    train = what == "train"
    leaves = (x, res, weight, bias)
    if train:
        for t in leaves:
            t.requires_grad_(True)
        up = torch.randn(B, S, hidden, device=DEV, generator=g).to(dtype)

    def forward(route):
        if route == "literal":
            return literal(x, res, weight, bias, P, train)
        return HF.residual_layer_norm(x, res, weight, bias, dropout_p=P, training=train, route=route)

    def call(route):
        def fn():
            if not train:
                with torch.no_grad():
                    return forward(route)
            for t in leaves:
                t.grad = None
            forward(route).backward(up)
        return fn

    row = {"kind": "tail", "what": what, "B": B, "S": S, "rows": B * S, "hidden": hidden,
           "dtype": str(dtype).replace("torch.", "")}
    for route in ("composed", "literal", "launch"):
        row[route] = summary(*windows(call(route), repeats, window_ms))
    with torch.no_grad():               # the routes must compute the same thing at the sizes timed
        a = HF.residual_layer_norm(x, res, weight, bias, route="launch").float()
        b = HF.residual_layer_norm(x, res, weight, bias, route="composed").float()
    row["rel_diff"] = float((a - b).abs().max() / b.abs().max())
    row["ahead"] = verdict(row["launch"], row["composed"], ("launch", "composed"))
    row["speedup"] = row["composed"]["median_ms"] / row["launch"]["median_ms"]
    row["speedup_over_literal"] = row["literal"]["median_ms"] / row["launch"]["median_ms"]
    if B == BATCHES[-1] and S == LENGTHS[-1] and hidden == WIDTHS[-1]:
        n, es = B * S * hidden, x.element_size()
        moved = 3 * n * es if not train else 7 * n * es + 2 * n          # keep: one byte, read forward and backward
        row["launch_bytes"] = moved
        row["launch_tb_per_s"] = moved / (row["launch"]["median_ms"] * 1e-3) / 1e12
        row["copy_tb_per_s"] = COPY_TBS
    return row


def layer(B, S, what, repeats, window_ms):
    torch.manual_seed(B)
    mod = BL.BertLayer(768, 12, 3072, hidden_dropout_prob=P, attention_probs_dropout_prob=P,
                       linear=BL.reference_tt_linear, layer_id=0).to(DEV)
    train = what == "train"
    mod.train(train)
    x = torch.randn(B, S, 768, device=DEV, requires_grad=train)
    mask = torch.zeros(B, 1, 1, S, device=DEV)
    for b in range(B):
        mask[b, 0, 0, S - (b * 7) % (S // 2):] = -10000.0 if b else 0.0
    up = torch.randn(B, S, 768, device=DEV)

    def call(route):
        def fn():
            mod.set_route(route)
            if not train:
                with torch.no_grad():
                    return mod(x, mask)
            mod.zero_grad(set_to_none=True)
            x.grad = None
            mod(x, mask)[0].backward(up)
        return fn

    row = {"kind": "layer", "what": what, "B": B, "S": S, "dtype": "float32"}
    for name, route in (("composed", "composed"), ("ruled", None)):
        row[name] = summary(*windows(call(route), repeats, window_ms))
    row["ahead"] = verdict(row["ruled"], row["composed"], ("ruled", "composed"))
    row["speedup"] = row["composed"]["median_ms"] / row["ruled"]["median_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--quick", action="store_true", help="B = 8 only")
    ap.add_argument("--skip-layer", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bertlayer.py needs the MI355X: a timing taken elsewhere says nothing")
    batches = (8,) if a.quick else BATCHES
    for dtype in (torch.float32, torch.bfloat16):
        for hidden in WIDTHS:
            for B in batches:
                for S in LENGTHS:
                    for what in ("fwd", "train"):
                        print(json.dumps(tail(B, S, hidden, dtype, what, a.repeats, a.window_ms)), flush=True)
            torch.cuda.empty_cache()
    if not a.skip_layer:
        for B in batches:
            for what in ("fwd", "train"):
                print(json.dumps(layer(B, 128, what, a.repeats, a.window_ms)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
