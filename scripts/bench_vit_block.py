"""The pre-norm block tail of a vision transformer, a whole TTBlock and the attention body at 197 tokens: the launches
(csrc/prenorm.hip, csrc/attn.hip) against the composed torch routes in the same run.

    python scripts/bench_vit_block.py [--repeats 5] [--window-ms 50] [--quick] [--skip-block] [--skip-attn]

Tail classes (`functional.add_layer_norm`): rows = 197 B for B in {1, 64, 256}, C in {192, 384, 768}, float32 and
bfloat16 (parameters in the type of x on both routes), a forward in eval mode under no_grad and a training step with
drop_path_p = 0.1 drawn by each route's own torch call, gradients into both outputs and from there into x, branch, weight
and bias.  For the largest class the bytes the launch has to move (forward: x, b, s, y; step: also g_s, g_y, s again, dx,
db) over its time stand next to the 6.29 TB/s copy rate.

Block classes: one TTBlock of DeiT-tiny (192, 3 heads) and one of DeiT-small (384, 6 heads) with the shipped TT-matrix
rank tables, float32, B in {1, 64}, 197 tokens, drop_path 0.1: every route forced to "launch" against every route forced
to "composed", forward and training step.

Attention classes (`functional.self_attention`, recorded only: `ops.attn_pays` is not changed from them): S = 197,
d = 64, H in {3, 6}, B in {1, 64}, float32 and bfloat16, q, k and v the column slices of a packed qkv tensor, no mask, no
scores, forward and training step.

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
from tadmm import get_hp_dict  # noqa: E402
from tadmm import vit_layers as VL  # noqa: E402

DEV = "cuda:0"
TOKENS = 197
BATCHES = (1, 64, 256)
WIDTHS = (192, 384, 768)
COPY_TBS = 6.29
P_PATH = 0.1


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


def both_routes(row, call, repeats, window_ms):
    for route in ("composed", "launch"):
        row[route] = summary(*windows(call(route), repeats, window_ms))
    row["ahead"] = verdict(row["launch"], row["composed"], ("launch", "composed"))
    row["speedup"] = row["composed"]["median_ms"] / row["launch"]["median_ms"]
    return row


def tail(B, C, dtype, what, repeats, window_ms):
    g = torch.Generator(device=DEV).manual_seed(B * 4099 + C)
    x, b = (torch.randn(B, TOKENS, C, device=DEV, generator=g).to(dtype) for _ in range(2))
    weight = (1 + 0.1 * torch.randn(C, device=DEV, generator=g)).to(dtype)
    bias = (0.1 * torch.randn(C, device=DEV, generator=g)).to(dtype)
    train = what == "train"
    leaves = (x, b, weight, bias)
    if train:
        for t in leaves:
            t.requires_grad_(True)
        ups = [torch.randn(B, TOKENS, C, device=DEV, generator=g).to(dtype) for _ in range(2)]

    def call(route):
        def fn():
            if not train:
                with torch.no_grad():
                    return HF.add_layer_norm(x, b, weight, bias, route=route)
            for t in leaves:
                t.grad = None
            s, y = HF.add_layer_norm(x, b, weight, bias, drop_path_p=P_PATH, training=True, route=route)
            torch.autograd.backward([s, y], ups)
        return fn

    row = {"kind": "tail", "what": what, "B": B, "rows": B * TOKENS, "hidden": C, "dtype": str(dtype).replace("torch.", "")}
    both_routes(row, call, repeats, window_ms)
    with torch.no_grad():               # the routes must compute the same thing at the sizes timed
        a = HF.add_layer_norm(x, b, weight, bias, route="launch")
        c = HF.add_layer_norm(x, b, weight, bias, route="composed")
    row["rel_diff"] = max(float((u.float() - v.float()).abs().max() / v.float().abs().max()) for u, v in zip(a, c))
    if B == BATCHES[-1] and C == WIDTHS[-1]:
        n, es = B * TOKENS * C, x.element_size()
        moved = (4 if not train else 9) * n * es
        row["launch_bytes"] = moved
        row["launch_tb_per_s"] = moved / (row["launch"]["median_ms"] * 1e-3) / 1e12
        row["copy_tb_per_s"] = COPY_TBS
    return row


def block(model, B, what, repeats, window_ms):
    dim, heads = {"deit_tiny": (192, 3), "deit_small": (384, 6)}[model]
    torch.manual_seed(B)
    hp = get_hp_dict(f"ttm_{model}_patch16_224", "2")
    mod = VL.TTBlock(dim, heads, qkv_bias=True, drop_path=P_PATH, norm_layer=lambda d: torch.nn.LayerNorm(d, eps=1e-6),
                     linear=VL.TTLinearM, block_id=0, hp_dict=hp).to(DEV)
    train = what == "train"
    mod.train(train)
    x = torch.randn(B, TOKENS, dim, device=DEV, requires_grad=train)
    up = torch.randn(B, TOKENS, dim, device=DEV)

    def call(route):
        def fn():
            mod.set_route(route)
            if not train:
                with torch.no_grad():
                    return mod(x)
            mod.zero_grad(set_to_none=True)
            x.grad = None
            mod(x).backward(up)
        return fn

    row = {"kind": "block", "model": model, "what": what, "B": B, "dtype": "float32"}
    return both_routes(row, call, repeats, window_ms)


def attention(B, H, dtype, what, repeats, window_ms):
    d = 64
    g = torch.Generator(device=DEV).manual_seed(B * 31 + H)
    train = what == "train"
    qkv = torch.randn(B, TOKENS, 3 * H * d, device=DEV, generator=g).to(dtype).requires_grad_(train)
    up = torch.randn(B, TOKENS, H * d, device=DEV, generator=g).to(dtype)

    def call(route):
        def fn():
            q, k, v = qkv[..., :H * d], qkv[..., H * d:2 * H * d], qkv[..., 2 * H * d:]
            if not train:
                with torch.no_grad():
                    return HF.self_attention(q, k, v, None, H, need_scores=False, route=route)
            qkv.grad = None
            HF.self_attention(q, k, v, None, H, need_scores=False, route=route)[0].backward(up)
        return fn

    row = {"kind": "attention", "what": what, "B": B, "H": H, "S": TOKENS, "d": d, "dtype": str(dtype).replace("torch.", "")}
    return both_routes(row, call, repeats, window_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--quick", action="store_true", help="B = 64 only")
    ap.add_argument("--skip-block", action="store_true")
    ap.add_argument("--skip-attn", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vit_block.py needs the MI355X: a timing taken elsewhere says nothing")
    batches = (64,) if a.quick else BATCHES
    for dtype in (torch.float32, torch.bfloat16):
        for C in WIDTHS:
            for B in batches:
                for what in ("fwd", "train"):
                    print(json.dumps(tail(B, C, dtype, what, a.repeats, a.window_ms)), flush=True)
            torch.cuda.empty_cache()
    if not a.skip_block:
        for model in ("deit_tiny", "deit_small"):
            for B in (64,) if a.quick else (1, 64):
                for what in ("fwd", "train"):
                    print(json.dumps(block(model, B, what, a.repeats, a.window_ms)), flush=True)
            torch.cuda.empty_cache()
    if not a.skip_attn:
        for dtype in (torch.float32, torch.bfloat16):
            for H in (3, 6):
                for B in (64,) if a.quick else (1, 64):
                    for what in ("fwd", "train"):
                        print(json.dumps(attention(B, H, dtype, what, a.repeats, a.window_ms)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
