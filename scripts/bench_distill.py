"""Distillation loss: the two-launch route (csrc/distill.hip) against the composed torch route, value only and value +
backward.

    python scripts/bench_distill.py [--repeats 7] [--iters 200]

The yardstick is `functional.distillation_loss_composed` where the checkout has it, else the function `yardstick` below,
which is the same lines written out (losses.py:35-61 of the reference: cross entropy, log_softmax, kl_div, argmax), so
this file runs unchanged on a checkout without the launch and then times the yardstick alone.  Shapes: DeiT (256 and
1024 rows of 1000 classes), CIFAR (128 rows of 10 / 100), TinyBERT's soft cross entropy (32 rows of 2 / 3).

Every figure: median of `--repeats` windows of `--iters` calls each, host clock around work that ends in a device
synchronise, after 3 warm-up calls per shape; min..max of the windows is the spread.  `ahead` is printed only when the
launch's max is below the yardstick's min (or the other way round), the rule every `*_pays` function follows.
"""
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

from tadmm import functional as HF  # noqa: E402

DEV = "cuda:0"
SHAPES = [(32, 2), (32, 3), (128, 10), (128, 100), (256, 1000), (1024, 1000)]


def yardstick(outputs, outputs_kd, teacher, target, *, kd, alpha=0.5, tau=3.0, **_):
    base = F.cross_entropy(outputs.float(), target)
    k, t = outputs_kd.float(), teacher.float()
    if kd == "soft":
        d = F.kl_div(F.log_softmax(k / tau, dim=1), F.log_softmax(t / tau, dim=1), reduction="sum",
                     log_target=True) * (tau * tau) / k.numel()
    else:
        d = F.cross_entropy(k, t.argmax(dim=1))
    return base * (1 - alpha) + d * alpha


def windows(fn, repeats, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters * 1e3)
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


def one(B, C, kd, dtype, grad, repeats, iters):
    g = torch.Generator(device=DEV).manual_seed(B * 4099 + C)
    s = (3 * torch.randn(B, C, device=DEV, generator=g)).to(dtype)
    k = (3 * torch.randn(B, C, device=DEV, generator=g)).to(dtype)
    t = (3 * torch.randn(B, C, device=DEV, generator=g)).to(dtype)
    y = torch.randint(0, C, (B,), device=DEV, generator=g)
    kw = dict(base="index", kd=kd, alpha=0.5, tau=3.0)
    if grad:
        s.requires_grad_(True)
        k.requires_grad_(True)

    def call(route_fn):
        def fn():
            if not grad:
                with torch.no_grad():
                    return route_fn(s, k, t, y, **kw)
            s.grad = k.grad = None
            route_fn(s, k, t, y, **kw).backward()
        return fn

    composed = getattr(HF, "distillation_loss_composed", yardstick)
    row = {"what": "train" if grad else "value", "B": B, "C": C, "kd": kd, "dtype": str(dtype).replace("torch.", "")}
    row["composed"] = summary(windows(call(composed), repeats, iters))
    launch = getattr(HF, "distillation_loss", None)
    if launch is not None:
        row["launch"] = summary(windows(call(lambda *a, **q: launch(*a, route="launch", **q)), repeats, iters))
        with torch.no_grad():       # the two routes must compute the same thing at the sizes timed
            la, lb = launch(s, k, t, y, route="launch", **kw), composed(s, k, t, y, **kw)
        row["rel_diff"] = abs(float(la) - float(lb)) / abs(float(lb))
        row["ahead"] = verdict(row["launch"], row["composed"])
        row["speedup"] = row["composed"]["median_ms"] / row["launch"]["median_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_distill.py needs the MI355X: a timing taken elsewhere says nothing")
    for B, C in SHAPES:
        for kd in ("soft", "hard"):
            for dtype in (torch.float32, torch.float16):
                for grad in (False, True):
                    print(json.dumps(one(B, C, kd, dtype, grad, a.repeats, a.iters)), flush=True)


if __name__ == "__main__":
    main()
