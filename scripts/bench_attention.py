"""BERT self-attention: the launch (csrc/attn.hip) against the composed torch route (`functional.self_attention_composed`,
the reference's nine calls), forward with and without the scores output and a training step with gradients into both
outputs.

    python scripts/bench_attention.py [--repeats 5] [--window-ms 50] [--quick]

Classes: H = 12, d = 64 (BERT-base), B in {1, 8, 32}, S in {64, 128, 384, 512}, float32 and bfloat16; an additive padding
mask as the reference builds it; dropout off (the keep mask would be drawn by the same torch call on both routes).

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dnn-compression-tensor-admm_amd"))

from tadmm import functional as HF  # noqa: E402

DEV = "cuda:0"
H, D = 12, 64
BATCHES = (1, 8, 32)
LENGTHS = (64, 128, 384, 512)


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


def verdict(a, b):
    """'launch' / 'composed' when one is ahead beyond the spread of both, else 'level'."""
    if a["max_ms"] < b["min_ms"]:
        return "launch"
    if b["max_ms"] < a["min_ms"]:
        return "composed"
    return "level"


def one(B, S, dtype, what, repeats, window_ms):
    g = torch.Generator(device=DEV).manual_seed(B * 4099 + S)
    q, k, v = (torch.randn(B, S, H * D, device=DEV, generator=g).to(dtype) for _ in range(3))
    mask = torch.zeros(B, 1, 1, S, device=DEV, dtype=dtype)
    for b in range(B):
        mask[b, 0, 0, S - (b * 7) % (S // 2):] = -10000.0 if b else 0.0
    train = what == "train"
    need_scores = what != "fwd_ctx"
    if train:
        for t in (q, k, v):
            t.requires_grad_(True)
        g_ctx = torch.randn(B, S, H * D, device=DEV, generator=g).to(dtype)
        g_sc = torch.randn(B, H, S, S, device=DEV, generator=g).to(dtype)

    def call(route):
        def fn():
            if not train:
                with torch.no_grad():
                    return HF.self_attention(q, k, v, mask, H, need_scores=need_scores, route=route)
            q.grad = k.grad = v.grad = None
            c, s = HF.self_attention(q, k, v, mask, H, route=route)
            torch.autograd.backward((c, s), (g_ctx, g_sc))
        return fn

    row = {"what": what, "B": B, "S": S, "dtype": str(dtype).replace("torch.", "")}
    for route in ("composed", "launch"):
        row[route] = summary(*windows(call(route), repeats, window_ms))
    with torch.no_grad():               # the two routes must compute the same thing at the sizes timed
        a = HF.self_attention(q, k, v, mask, H, route="launch")[0].float()
        b = HF.self_attention(q, k, v, mask, H, route="composed")[0].float()
    row["rel_diff"] = float((a - b).abs().max() / b.abs().max())
    row["ahead"] = verdict(row["launch"], row["composed"])
    row["speedup"] = row["composed"]["median_ms"] / row["launch"]["median_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--quick", action="store_true", help="B = 8 only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention.py needs the MI355X: a timing taken elsewhere says nothing")
    for dtype in (torch.float32, torch.bfloat16):
        for B in ((8,) if a.quick else BATCHES):
            for S in LENGTHS:
                for what in ("fwd_scores", "fwd_ctx", "train"):
                    print(json.dumps(one(B, S, dtype, what, a.repeats, a.window_ms)), flush=True)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
