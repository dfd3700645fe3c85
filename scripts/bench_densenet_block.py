"""The pre-activation of a DenseNet layer and whole dense blocks of the CIFAR and ImageNet DenseNets: the launch
(csrc/densebn.hip) against the composed torch route (torch.cat + F.batch_norm + relu) in the same run.

    python scripts/bench_densenet_block.py [--repeats 5] [--window-ms 50] [--quick] [--skip-block]

Layer classes (`functional.dense_batch_norm_act`), (N, feature tensors, C, H W): the first, middle and last layer of each
block, every transition and the final norm of DenseNet-40 (growth 16, twelve basic layers per block, planes 32, 16, 8;
N in {1, 128}) and of DenseNet-121 (growth 32, blocks of 6, 12, 24, 16 layers, planes 56, 28, 14, 7; N in {1, 32}); the
first feature tensor is the block's input, every other one has `growth` channels.  float32 and bfloat16 (parameters and
running statistics float32 on both routes); a forward in eval mode under no_grad and a training step (forward in training
mode, gradients into every feature tensor, weight and bias).  In the training step the launch route is timed as a layer
inside a block pays for it: the batch statistics of every feature tensor but the newest are already with the
`DenseFeatures` (earlier layers computed them), those of the newest are computed in the timed call.  A first layer has
one feature tensor and computes its statistics itself.

Block classes: block 1 of tkr_densenet40 (12 basic layers, 32 channels in, 32 x 32, N = 128, TKConv2dR from the shipped
table) and denseblock1 of tkc_densenet121 (6 layers, 64 channels in, 56 x 56, N = 32, TKConv2dC from the shipped table),
float32, every BatchNorm forced to "launch" against every BatchNorm forced to "composed", training step with a gradient
arriving at every feature tensor the block made.

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

from tadmm import densenet_cifar_layers as DC  # noqa: E402
from tadmm import densenet_inet_layers as DI  # noqa: E402
from tadmm import functional as HF  # noqa: E402
from tadmm import get_hp_dict  # noqa: E402

DEV = "cuda:0"


def layer_classes(c_in, growth, layers, sides, last_name):
    """(where, feature tensors, first tensor's channels, growth, plane side) of the first, middle and last layer of every
    block, of every transition and of the final norm."""
    out = []
    for b, (nl, side) in enumerate(zip(layers, sides), 1):
        for i in (0, nl // 2, nl - 1):
            out.append((f"block{b}.layer{i}", i + 1, c_in, growth, side))
        where = f"trans{b}" if b < len(layers) else last_name
        out.append((where, nl + 1, c_in, growth, side))
        c_in = (c_in + nl * growth) // 2
    return out


NETS = {
    "densenet40": (layer_classes(32, 16, (12, 12, 12), (32, 16, 8), "bn1"), (1, 128)),
    "densenet121": (layer_classes(64, 32, (6, 12, 24, 16), (56, 28, 14, 7), "norm5"), (1, 32)),
}


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


def layer(net, where, n, nseg, c_first, growth, side, dtype, what, repeats, window_ms):
    g = torch.Generator(device=DEV).manual_seed(n * 4099 + nseg)
    train = what == "train"
    chans = [c_first] + [growth] * (nseg - 1)
    c = sum(chans)
    segs = [torch.randn(n, ck, side, side, device=DEV, generator=g).to(dtype).requires_grad_(train) for ck in chans]
    weight = (1 + 0.1 * torch.randn(c, device=DEV, generator=g)).requires_grad_(train)
    bias = (0.1 * torch.randn(c, device=DEV, generator=g)).requires_grad_(train)
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    up = torch.randn(n, c, side, side, device=DEV, generator=g).to(dtype)
    leaves = segs + [weight, bias]
    feats = HF.DenseFeatures(segs)

    def call(route):
        def fn():
            if not train:
                with torch.no_grad():
                    return HF.dense_batch_norm_act(feats, rm, rv, weight, bias, training=False, route=route)
            for t in leaves:
                t.grad = None
            feats._stats[-1] = None                     # the newest feature tensor's statistics are this layer's work
            HF.dense_batch_norm_act(feats, rm, rv, weight, bias, training=True, route=route).backward(up)
        return fn

    row = {"kind": "layer", "net": net, "where": where, "what": what, "N": n, "nseg": nseg, "C": c, "HW": side * side,
           "dtype": str(dtype).replace("torch.", "")}
    both_routes(row, call, repeats, window_ms)
    with torch.no_grad():               # the routes must compute the same thing at the sizes timed
        a, b = (HF.dense_batch_norm_act(feats, rm.clone(), rv.clone(), weight, bias, training=train, route=r).float()
                for r in ("launch", "composed"))
    row["rel_diff"] = float((a - b).abs().max() / b.abs().max())
    return row


def make_block(which):
    if which == "densenet40.block1":
        hp = get_hp_dict("tkr_densenet40", "2")
        return DC.TenDenseBlock(12, 32, 16, DC.TenBasicBlock, conv=DC.TKConv2dR, stage=1, hp_dict=hp), (128, 32, 32)
    hp = get_hp_dict("tkc_densenet121", "2")
    return DI.TenDenseBlock(6, 64, 4, 32, stage=1, hp_dict=hp), (32, 64, 56)


def block(which, repeats, window_ms):
    torch.manual_seed(1)
    mod, (n, c, side) = make_block(which)
    mod = mod.to(DEV).train()
    x = torch.randn(n, c, side, side, device=DEV, requires_grad=True)
    with torch.no_grad():
        made = list(mod.set_route("composed")(x))[1:]
    ups = [torch.randn_like(t) for t in made]

    def call(route):
        def fn():
            mod.set_route(route)
            mod.zero_grad(set_to_none=True)
            x.grad = None
            torch.autograd.backward(list(mod(x))[1:], ups)
        return fn

    row = {"kind": "block", "block": which, "what": "train", "N": n, "C": c, "HW": side * side, "layers": len(made),
           "dtype": "float32"}
    return both_routes(row, call, repeats, window_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--quick", action="store_true", help="the larger batch of each network only")
    ap.add_argument("--skip-block", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_densenet_block.py needs the MI355X: a timing taken elsewhere says nothing")
    for net, (classes, batches) in NETS.items():
        for where, nseg, c_first, growth, side in classes:
            for n in batches[1:] if a.quick else batches:
                for dtype in (torch.float32, torch.bfloat16):
                    for what in ("fwd", "train"):
                        print(json.dumps(layer(net, where, n, nseg, c_first, growth, side, dtype, what, a.repeats,
                                               a.window_ms)), flush=True)
            torch.cuda.empty_cache()
    if not a.skip_block:
        for which in ("densenet40.block1", "densenet121.denseblock1"):
            print(json.dumps(block(which, a.repeats, a.window_ms)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
