"""The depthwise stage of a MobileNetV2 block and whole blocks of the CIFAR and ImageNet MobileNetV2s: the launch
(csrc/dwbn.hip) against the composed torch route in the same run.

    python scripts/bench_mobilenet_block.py [--repeats 5] [--window-ms 50] [--quick] [--skip-block]

Stage classes (`functional.depthwise_bn_relu6`), (C, H = W, stride): CIFAR N in {1, 128} at (32, 32, 1), (96, 32, 1),
(144, 32, 1), (192, 32, 2), (384, 16, 1), (576, 16, 2), (960, 8, 1); ImageNet N in {1, 32} at (32, 112, 1), (96, 112, 2),
(144, 56, 2), (192, 28, 1), (384, 14, 1), (576, 14, 2), (960, 7, 1); float32 and bfloat16 (filter, parameters and running
statistics float32 on both routes); a forward in eval mode under no_grad and a training step (forward in training mode,
gradients into x, the filter, weight and bias).  Next to each launch stand the bytes it has to move (eval: x and y;
step: x three times -- forward, dw, dx -- and nine passes over the output plane: z written and read, y written, then g,
y, z read twice) over its time, against the 6.29 TB/s copy rate.

Block classes: the CIFAR TTBaseBlock 4 (32 -> 32 with shortcut, 192 wide at 32 x 32, svd table, SVDConv2dC) and the
ImageNet TTInvertedResidual `features.8` (64 -> 64 with identity, 384 wide at 14 x 14, svd table, SVDConv2dM), float32,
the depthwise stage and the bottleneck tail forced to "launch" against both forced to "composed", forward and training
step.

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
from tadmm import get_hp_dict, ops  # noqa: E402
from tadmm import mobilenet_cifar_layers as MC  # noqa: E402
from tadmm import mobilenet_inet_layers as MI  # noqa: E402

DEV = "cuda:0"
COPY_TBS = 6.29
CIFAR = [(n, c, h, s) for c, h, s in ((32, 32, 1), (96, 32, 1), (144, 32, 1), (192, 32, 2), (384, 16, 1), (576, 16, 2),
                                      (960, 8, 1)) for n in (1, 128)]
INET = [(n, c, h, s) for c, h, s in ((32, 112, 1), (96, 112, 2), (144, 56, 2), (192, 28, 1), (384, 14, 1), (576, 14, 2),
                                     (960, 7, 1)) for n in (1, 32)]


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


def stage(net, n, c, side, stride, dtype, what, repeats, window_ms):
    g = torch.Generator(device=DEV).manual_seed(n * 4099 + c)
    train = what == "train"
    x = torch.randn(n, c, side, side, device=DEV, generator=g).to(dtype).requires_grad_(train)
    filt = (torch.randn(c, 1, 3, 3, device=DEV, generator=g) / 3).requires_grad_(train)
    weight = (1 + 0.1 * torch.randn(c, device=DEV, generator=g)).requires_grad_(train)
    bias = (0.1 * torch.randn(c, device=DEV, generator=g)).requires_grad_(train)
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    ho, wo = ops.dwbn_out_hw(side, side, stride)
    up = torch.randn(n, c, ho, wo, device=DEV, generator=g).to(dtype)
    leaves = (x, filt, weight, bias)

    def call(route):
        def fn():
            if not train:
                with torch.no_grad():
                    return HF.depthwise_bn_relu6(x, filt, rm, rv, weight, bias, stride=stride, training=False, route=route)
            for t in leaves:
                t.grad = None
            HF.depthwise_bn_relu6(x, filt, rm, rv, weight, bias, stride=stride, training=True, route=route).backward(up)
        return fn

    row = {"kind": "stage", "net": net, "what": what, "N": n, "C": c, "H": side, "stride": stride,
           "dtype": str(dtype).replace("torch.", "")}
    both_routes(row, call, repeats, window_ms)
    with torch.no_grad():               # the routes must compute the same thing at the sizes timed
        a, b = (HF.depthwise_bn_relu6(x, filt, rm.clone(), rv.clone(), weight, bias, stride=stride, training=train,
                                      route=r).float() for r in ("launch", "composed"))
    row["rel_diff"] = float((a - b).abs().max() / b.abs().max())
    moved = ((x.numel() + up.numel()) if not train else (3 * x.numel() + 9 * up.numel())) * x.element_size()
    row["launch_bytes"] = moved
    row["launch_tb_per_s"] = moved / (row["launch"]["median_ms"] * 1e-3) / 1e12
    row["copy_tb_per_s"] = COPY_TBS
    return row


def make_block(which):
    if which == "cifar_bottleneck4":
        hp = get_hp_dict("svdc_mobilenetv2_cifar", "2")
        return MC.TTBaseBlock(32, 32, conv=MC.SVDConv2dC, id=4, hp_dict=hp), (32, 32)
    hp = get_hp_dict("svdm_mobilenetv2", "2")
    return MI.TTInvertedResidual(64, 64, 1, 6, id=8, conv=MI.SVDConv2dM, hp_dict=hp), (64, 14)


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

    row = {"kind": "block", "block": which, "what": what, "N": n, "C": c, "H": side, "dtype": "float32"}
    return both_routes(row, call, repeats, window_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--quick", action="store_true", help="the larger batch of each network only")
    ap.add_argument("--skip-block", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mobilenet_block.py needs the MI355X: a timing taken elsewhere says nothing")
    for net, classes in (("cifar", CIFAR), ("imagenet", INET)):
        for n, c, side, stride in classes:
            if a.quick and n == 1:
                continue
            for dtype in (torch.float32, torch.bfloat16):
                for what in ("fwd", "train"):
                    print(json.dumps(stage(net, n, c, side, stride, dtype, what, a.repeats, a.window_ms)), flush=True)
            torch.cuda.empty_cache()
    if not a.skip_block:
        for which, batches in (("cifar_bottleneck4", (1, 128)), ("inet_features8", (1, 32))):
            for n in batches[1:] if a.quick else batches:
                for what in ("fwd", "train"):
                    print(json.dumps(block(which, n, what, a.repeats, a.window_ms)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
