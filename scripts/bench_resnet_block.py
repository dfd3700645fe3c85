"""The BatchNorm tail of a ResNet block and whole blocks of the CIFAR and ImageNet ResNets: the launch (csrc/bnact.hip)
against the composed torch route in the same run.

    python scripts/bench_resnet_block.py [--repeats 5] [--window-ms 50] [--quick] [--skip-block]

Tail classes (`functional.batch_norm_act`), (N, C, H W): CIFAR N in {1, 128} at (16, 32^2), (32, 16^2), (64, 8^2);
ImageNet N in {1, 32} at (64, 56^2), (256, 56^2), (512, 28^2), (2048, 7^2); float32 and bfloat16 (parameters and running
statistics float32 on both routes); without a residual, with a full-width one and, for the two CIFAR classes that have
it, with the option-A window x_in[:, :, ::2, ::2] at channel offset C / 4 (composed: slice, F.pad, add); a forward in
eval mode under no_grad and a training step (forward in training mode, gradients into x, weight, bias and the residual).
For the largest class of each network the bytes the launch has to move (eval: x, res, y; step: x twice, res, y, then g, y,
x twice each and dx, dres) over its time stand next to the 6.29 TB/s copy rate.

Block classes: a CIFAR TTBasicBlock (stage 2, id 1, 32 planes at 16 x 16, tkc_resnet32 table), an ImageNet TTBasicBlock
(stage 2, id 1, 128 planes at 28 x 28, ttm_resnet18 table) and a TTBottleneck (stage 2, id 1, 512 channels at 28 x 28,
ttr_resnet50 general table), float32, every tail forced to "launch" against every tail forced to "composed", forward
and training step.

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
from tadmm import resnet_cifar_layers as RC  # noqa: E402
from tadmm import resnet_inet_layers as RI  # noqa: E402

DEV = "cuda:0"
COPY_TBS = 6.29
CIFAR = [(n, c, s) for c, s in ((16, 32), (32, 16), (64, 8)) for n in (1, 128)]
INET = [(n, c, s) for c, s in ((64, 56), (256, 56), (512, 28), (2048, 7)) for n in (1, 32)]
LARGEST = {(128, 16, 32), (32, 256, 56)}


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


def both_routes(row, call, repeats, window_ms):
    for route in ("composed", "launch"):
        row[route] = summary(*windows(call(route), repeats, window_ms))
    a, b = row["launch"], row["composed"]
    row["ahead"] = "launch" if a["max_ms"] < b["min_ms"] else "composed" if b["max_ms"] < a["min_ms"] else "level"
    row["speedup"] = b["median_ms"] / a["median_ms"]
    return row


def tail(net, n, c, side, dtype, res_kind, what, repeats, window_ms):
    g = torch.Generator(device=DEV).manual_seed(n * 4099 + c)
    train = what == "train"
    x = torch.randn(n, c, side, side, device=DEV, generator=g).to(dtype).requires_grad_(train)
    weight = (1 + 0.1 * torch.randn(c, device=DEV, generator=g)).requires_grad_(train)
    bias = (0.1 * torch.randn(c, device=DEV, generator=g)).requires_grad_(train)
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    base, c0 = None, 0
    if res_kind == "full":
        base = torch.randn(n, c, side, side, device=DEV, generator=g).to(dtype).requires_grad_(train)
    elif res_kind == "optionA":
        base = torch.randn(n, c // 2, 2 * side, 2 * side, device=DEV, generator=g).to(dtype).requires_grad_(train)
        c0 = c // 4
    up = torch.randn(n, c, side, side, device=DEV, generator=g).to(dtype)
    leaves = [t for t in (x, weight, bias, base) if t is not None]

    def residual():
        return base[:, :, ::2, ::2] if res_kind == "optionA" else base

    def call(route):
        def fn():
            if not train:
                with torch.no_grad():
                    return HF.batch_norm_act(x, rm, rv, weight, bias, residual(), res_channel_offset=c0, training=False,
                                             route=route)
            for t in leaves:
                t.grad = None
            HF.batch_norm_act(x, rm, rv, weight, bias, residual(), res_channel_offset=c0, training=True,
                              route=route).backward(up)
        return fn

    row = {"kind": "tail", "net": net, "what": what, "N": n, "C": c, "HW": side * side, "residual": res_kind,
           "dtype": str(dtype).replace("torch.", "")}
    both_routes(row, call, repeats, window_ms)
    with torch.no_grad():               # the routes must compute the same thing at the sizes timed
        a, b = (HF.batch_norm_act(x, rm.clone(), rv.clone(), weight, bias, residual(), res_channel_offset=c0, training=train,
                                  route=r).float() for r in ("launch", "composed"))
    row["rel_diff"] = float((a - b).abs().max() / b.abs().max())
    if (n, c, side) in LARGEST and res_kind == "full":
        moved = (3 if not train else 13) * x.numel() * x.element_size()
        row["launch_bytes"] = moved
        row["launch_tb_per_s"] = moved / (row["launch"]["median_ms"] * 1e-3) / 1e12
        row["copy_tb_per_s"] = COPY_TBS
    return row


def make_block(which):
    if which == "cifar_basic":
        hp = get_hp_dict("tkc_resnet32", "3")
        return RC.TTBasicBlock(32, 32, 1, conv=RC.TKConv2dC, stage=2, id=1, hp_dict=hp), (32, 16)
    if which == "inet_basic":
        hp = get_hp_dict("ttm_resnet18", "2")
        return RI.TTBasicBlock(128, 128, stage=2, id=1, conv=RI.TTConv2dM, hp_dict=hp), (128, 28)
    hp = get_hp_dict("ttr_resnet50", "3", tt_type="general")
    return RI.TTBottleneck(512, 128, stage=2, id=1, conv=RI.TTConv2dR, hp_dict=hp), (512, 28)


def block(which, n, what, repeats, window_ms):
    torch.manual_seed(n)
    mod, (c, side) = make_block(which)
    mod = mod.to(DEV)
    train = what == "train"
    mod.train(train)
    x = torch.randn(n, c, side, side, device=DEV, requires_grad=train)
    up = torch.randn(n, c, side, side, device=DEV)

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

    row = {"kind": "block", "block": which, "what": what, "N": n, "C": c, "HW": side * side, "dtype": "float32"}
    return both_routes(row, call, repeats, window_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--quick", action="store_true", help="the larger batch of each network only")
    ap.add_argument("--skip-block", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resnet_block.py needs the MI355X: a timing taken elsewhere says nothing")
    for net, classes in (("cifar", CIFAR), ("imagenet", INET)):
        for n, c, side in classes:
            if a.quick and n == 1:
                continue
            kinds = ["none", "full"] + (["optionA"] if net == "cifar" and c > 16 else [])
            for dtype in (torch.float32, torch.bfloat16):
                for res_kind in kinds:
                    for what in ("fwd", "train"):
                        print(json.dumps(tail(net, n, c, side, dtype, res_kind, what, a.repeats, a.window_ms)), flush=True)
            torch.cuda.empty_cache()
    if not a.skip_block:
        for which, batches in (("cifar_basic", (1, 128)), ("inet_basic", (1, 32)), ("inet_bottleneck", (1, 32))):
            for n in batches[1:] if a.quick else batches:
                for what in ("fwd", "train"):
                    print(json.dumps(block(which, n, what, a.repeats, a.window_ms)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
