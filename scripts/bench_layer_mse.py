"""TinyBERT's layer losses: the two-launch route (csrc/layermse.hip) against the composed torch route, value only and
value + backward, in one run.

    python scripts/bench_layer_mse.py [--repeats 7] [--iters 200]

The yardstick is `functional.intermediate_distillation_loss_composed` (torch.where and F.mse_loss under autograd, one
mse_loss per pair: fewer launches than the reference's loop over the batch axis).  Shapes: the reference's step (the last
layer of a 12-head model at batch 32, 128 tokens: one attention pair and one hidden pair, reduction "batch_sum"), a small
step, and upstream TinyBERT's per-layer loops (4 + 5 and 12 + 13 pairs, reduction "mean").  Scores are randn plus a
-10000 mask over the last 30 % of the keys, so the clamp is at work.

Every figure: median of `--repeats` windows of `--iters` calls each, host clock around work that ends in a device
synchronise, after 3 warm-up calls per shape and route, the windows of the two routes alternating; min..max of the
windows is the spread.  `ahead` is printed only when one
side's max is below the other's min, the rule every `*_pays` function follows.  For the training step the row also
carries the bytes the launch has to move -- two reads in the tensors' type and one float32 write per element -- divided
by its median time; the chip's HBM ceiling is about 6.3 TB/s.  That figure is recorded, not gated, and it charges the
whole step (the backward's scaling pass included) to the forward's traffic.
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

from tadmm import functional as HF  # noqa: E402

DEV = "cuda:0"
# (name, attention pairs, (B, H, S), hidden pairs, (B, S, D), reduction)
CLASSES = [
    ("step-32x12x128", 1, (32, 12, 128), 1, (32, 128, 768), "batch_sum"),
    ("step-8x12x64", 1, (8, 12, 64), 1, (8, 64, 312), "batch_sum"),
    ("layers-4+5", 4, (32, 12, 128), 5, (32, 128, 312), "mean"),
    ("layers-12+13", 12, (8, 12, 128), 13, (8, 128, 768), "mean"),
]


def windows(fns, repeats, iters):
    """Per function the times of its `repeats` windows; the windows of the functions alternate, so that whatever else
    the host does meets both routes alike."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / iters * 1e3)
    return out


def summary(ws):
    return {"median_ms": statistics.median(ws), "min_ms": min(ws), "max_ms": max(ws)}


def verdict(a, b):
    """'launch' / 'composed' when one is ahead beyond the spread of both, else 'level'."""
    if a["max_ms"] < b["min_ms"]:
        return "launch"
    if b["max_ms"] < a["min_ms"]:
        return "composed"
    return "level"


def one(name, natt, att_shape, nrep, rep_shape, reduction, dtype, grad, repeats, iters):
    g = torch.Generator(device=DEV).manual_seed(natt * 131 + nrep)
    B, H, S = att_shape
    mask = torch.zeros(B, 1, 1, S, device=DEV)
    mask[..., S - (3 * S) // 10:] = -10000.0
    draw = lambda *shape: torch.randn(*shape, device=DEV, generator=g)
    sa = [(draw(B, H, S, S) + mask).to(dtype) for _ in range(natt)]
    ta = [(draw(B, H, S, S) + mask).to(dtype) for _ in range(natt)]
    sr = [draw(*rep_shape).to(dtype) for _ in range(nrep)]
    tr = [draw(*rep_shape).to(dtype) for _ in range(nrep)]
    students = sa + sr
    if grad:
        for s in students:
            s.requires_grad_(True)

    def call(route_fn):
        def fn():
            if not grad:
                with torch.no_grad():
                    return route_fn(sa, ta, sr, tr, reduction=reduction)
            for s in students:
                s.grad = None
            att, rep = route_fn(sa, ta, sr, tr, reduction=reduction)
            (att + rep).backward()
        return fn

    composed = HF.intermediate_distillation_loss_composed
    launch = lambda *a, **q: HF.intermediate_distillation_loss(*a, route="launch", **q)
    elems = sum(s.numel() for s in students)
    row = {"what": "train" if grad else "value", "class": name, "pairs": natt + nrep, "elements": elems,
           "dtype": str(dtype).replace("torch.", ""), "reduction": reduction}
    wc, wl = windows([call(composed), call(launch)], repeats, iters)
    row["composed"], row["launch"] = summary(wc), summary(wl)
    with torch.no_grad():       # the two routes must compute the same thing at the sizes timed
        la, lb = launch(sa, ta, sr, tr, reduction=reduction), composed(sa, ta, sr, tr, reduction=reduction)
    row["rel_diff"] = max(abs(float(x) - float(y)) / abs(float(y)) for x, y in zip(la, lb))
    row["ahead"] = verdict(row["launch"], row["composed"])
    row["speedup"] = row["composed"]["median_ms"] / row["launch"]["median_ms"]
    if grad:
        moved = elems * (2 * sa[0].element_size() + 4)
        row["launch_bytes"] = moved
        row["launch_TB_per_s"] = moved / (row["launch"]["median_ms"] * 1e-3) / 1e12
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_layer_mse.py needs the MI355X: a timing taken elsewhere says nothing")
    for cls in CLASSES:
        for dtype in (torch.float32, torch.bfloat16):
            for grad in (False, True):
                print(json.dumps(one(*cls, dtype, grad, a.repeats, a.iters)), flush=True)


if __name__ == "__main__":
    main()
