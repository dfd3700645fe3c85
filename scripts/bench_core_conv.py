"""The k x k core convolution of the factorised layers at the shapes of their tables: the 3 x 3 cores of resnet18_tt 2x,
resnet50_tt 3x, tk_resnet50 3x (batch 32, ImageNet planes) and tk_resnet32 3x (batch 128, CIFAR planes), fp32 and bf16,
forward alone and forward + backward.  Layers with the same (r1, r2, plane, stride) are timed once.

Paths:  native -- tadmm_core_conv_fwd (+ tadmm_core_conv_dgrad + tadmm_core_conv_wgrad), `HF.core_conv`
        lib    -- F.conv2d of the device library with the same operands (what the layers ran before): the yardstick
Timing: HIP events around `ITERS` calls after a warm-up, ROUNDS rounds with the order of the paths rotated every round;
the median and the spread (min..max) of the rounds are reported.  `ahead` is true when the native median is below the
library's fastest round, false when it is above its slowest, null inside the library's own spread.

    python scripts/bench_core_conv.py [--quick] [--json OUT]
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

from tadmm import functional as HF  # noqa: E402
from tadmm import hp, workloads  # noqa: E402

DEV = torch.device("cuda", 0)
TABLES = (("tt_resnet18_hp.HyperParamsDictGeneralRatio2x", 32), ("tt_resnet50_hp.HyperParamsDictGeneralRatio3x", 32),
          ("tk_resnet50_hp.HyperParamsDictRatio3x", 32), ("tk_resnet32_hp.HyperParamsDictRatio3x", 128))


def geometry(key, name):
    """(input plane side, stride) of a 3 x 3 kernel of resnet18 / resnet50 (ImageNet) or resnet32 (CIFAR)."""
    layer, block, conv = int(name[5]), int(name.split(".")[1]), name.split(".")[2]
    if "_resnet32_" in key:
        side = {1: 32, 2: 16, 3: 8}[layer]
        strided = layer > 1 and block == 0 and conv == "conv1"
    else:
        side = {1: 56, 2: 28, 3: 14, 4: 7}[layer]
        strided = layer > 1 and block == 0 and conv == ("conv2" if "_resnet50_" in key else "conv1")
    return (side * 2, 2) if strided else (side, 1)


def shapes():
    seen, out = set(), []
    for key, batch in TABLES:
        table = hp.fresh_table(key)
        fn = workloads.shape_fn_for(key)
        for name, ranks in table.ranks.items():
            shp = fn(name)
            if len(shp) != 4 or shp[2] == 1 or not name.startswith("layer"):
                continue
            if key.startswith("tt_"):
                kq = list(table.tt_shapes[name]).index(shp[2] * shp[3])
                r2, r1 = ranks[kq], ranks[kq + 1]
            else:
                r2, r1 = ranks[0], ranks[1]
            side, stride = geometry(key, name)
            sig = (batch, r1, r2, side, shp[2], stride)
            if sig not in seen:
                seen.add(sig)
                out.append((key.split("_hp")[0], name) + sig)
    return out


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(paths, iters, rounds):
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    names = list(paths)
    res = {n: [] for n in names}
    for k in range(rounds):
        order = names[k % len(names):] + names[:k % len(names)]
        for n in order:
            res[n].append(timed(paths[n], iters))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in res.items()}


def bench_shape(table, name, B, r1, r2, side, k, stride, dtype, train, iters, rounds):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, r1, side, side, generator=g).to(DEV).to(dtype)
    core = (torch.randn(r2, r1, k, k, generator=g) * (r1 * k * k) ** -0.5).to(DEV)
    core_c = core.to(dtype)
    pad = k // 2
    if not train:
        cache = {}
        paths = {"native": lambda: HF.core_conv(x, core, stride, pad, 1, cache=cache),
                 "lib": lambda: F.conv2d(x, core_c, None, stride, pad)}
        ctx = torch.no_grad()
    else:
        xg, cg = x.clone().requires_grad_(), core.clone().requires_grad_()
        xl, cl = x.clone().requires_grad_(), core_c.clone().requires_grad_()
        side_o = (side + 2 * pad - k) // stride + 1
        gy = torch.randn(B, r2, side_o, side_o, generator=g).to(DEV).to(dtype)
        paths = {"native": lambda: HF.core_conv(xg, cg, stride, pad, 1).backward(gy),
                 "lib": lambda: F.conv2d(xl, cl, None, stride, pad).backward(gy)}
        ctx = torch.enable_grad()
    with ctx:
        t = measure(paths, iters, rounds)
    row = dict(table=table, layer=name, B=B, r1=r1, r2=r2, side=side, k=k, stride=stride, dtype=str(dtype)[6:],
               mode="fwd+bwd" if train else "fwd")
    for p, (med, lo, hi) in t.items():
        row[p + "_ms"] = round(med, 4)
        row[p + "_spread"] = [round(lo, 4), round(hi, 4)]
    row["lib_over_native"] = round(t["lib"][0] / t["native"][0], 3)
    row["ahead"] = True if t["native"][0] < t["lib"][1] else False if t["native"][0] > t["lib"][2] else None
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer iterations and rounds")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    iters, rounds = (5, 3) if a.quick else (20, 5)
    rows = []
    for table, name, B, r1, r2, side, k, stride in shapes():
        for dtype in (torch.float32, torch.bfloat16):
            for train in (False, True):
                row = bench_shape(table, name, B, r1, r2, side, k, stride, dtype, train, iters, rounds)
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
