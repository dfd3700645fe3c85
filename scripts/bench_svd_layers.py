"""The 1x1 SVD layers (SVDConv2dC / SVDConv2dM) at the shapes of their tables: every layer of svd_mobilenetv2_cifar 2x at
batch 128 and the single-rank layers of tk_resnet50 3x at batch 64, fp32 and bf16, inference and forward + backward.

Paths:  fused  -- one tadmm_svdconv_fwd launch (backward: tadmm_svdconv_bwd + two single products + two GEMMs)
        two    -- two tadmm_tucker_1x1 launches (the r-channel intermediate goes through HBM)
        ref    -- the reference composition, two F.conv2d
        dense  -- F.conv2d with the recovered (O, I) weight
Timing: HIP events around `ITERS` calls after a warm-up, ROUNDS rounds with the order of the paths rotated every round;
the median and the spread (min..max) of the rounds are reported.  `bw_share` = bytes that must move (x in, y out, plus the
intermediate written and read again for `two`) / 8 TB/s, divided by the measured time.

    python scripts/bench_svd_layers.py [--quick] [--json OUT]
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

HBM_BPS = 8.0e12
DEV = torch.device("cuda", 0)


def mbv2_cifar_plane(name):
    """Plane side of a 1x1 kernel of mobilenetv2_cifar.py (32x32 input, downsampling blocks 6 and 13)."""
    if name == "conv1.weight":
        return 8
    i, conv = int(name.split(".")[1]), name.split(".")[2]
    side = 32 if i < 6 else 16 if i < 13 else 8
    if i in (6, 13) and conv == "conv3":
        side //= 2
    return side


def resnet50_plane(name):
    layer, block, conv = int(name[5]), int(name.split(".")[1]), name.split(".")[2]
    side = {1: 56, 2: 28, 3: 14, 4: 7}[layer]
    if conv == "conv1" and block == 0 and layer > 1:
        side *= 2                                   # the first 1x1 of a downsampling block runs before the stride
    return side


def layers():
    out = []
    for key, batch, plane in (("svd_mobilenetv2_cifar_hp.HyperParamsDictRatio2x", 128, mbv2_cifar_plane),
                              ("tk_resnet50_hp.HyperParamsDictRatio3x", 64, resnet50_plane)):
        table = hp.fresh_table(key)
        fn = workloads.shape_fn_for(key)
        for name, r in table.ranks.items():
            r = r if isinstance(r, int) else (r[0] if len(r) == 1 else None)
            if r is None:
                continue
            o, i = fn(name)[:2]
            out.append((key.split("_hp")[0], name, batch, i, o, r, plane(name)))
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


def bench_layer(table, name, B, cin, cout, r, side, dtype, train, iters, rounds):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, cin, side, side, generator=g).to(DEV).to(dtype)
    w_in = (torch.randn(r, cin, generator=g) / cin ** 0.5).to(DEV)
    w_out = (torch.randn(cout, r, generator=g) / r ** 0.5).to(DEV)
    bias = torch.randn(cout, generator=g).to(DEV)
    n = 1 if dtype == torch.bfloat16 else 3
    wi_c, wo_c, b_c = w_in.to(dtype), w_out.to(dtype), bias.to(dtype)
    dense_w = (w_out @ w_in).to(dtype)[:, :, None, None]
    paths = {}
    if not train:
        planes = (HF.planes_of(w_in, n, pad_rows=64), HF.planes_of(w_out, n, pad_cols=64))
        p1, p2 = HF.planes_of(w_in, n), HF.planes_of(w_out, n)
        if r <= 256:
            paths["fused"] = lambda: HF.conv1x1_chain(x, w_in, w_out, bias, planes)
        paths["two"] = lambda: HF.pointwise(HF.pointwise(x, w_in, None, "tadmm_tucker_1x1", p1), w_out, bias,
                                            "tadmm_tucker_1x1", p2)
        paths["ref"] = lambda: F.conv2d(F.conv2d(x, wi_c[:, :, None, None]), wo_c[:, :, None, None], b_c)
        paths["dense"] = lambda: F.conv2d(x, dense_w, b_c)
        ctx = torch.no_grad()
    else:
        xg = x.clone().requires_grad_()
        wi, wo, bb = w_in.clone().requires_grad_(), w_out.clone().requires_grad_(), bias.clone().requires_grad_()
        wic, woc, bc = wi_c.clone().requires_grad_(), wo_c.clone().requires_grad_(), b_c.clone().requires_grad_()
        wd = dense_w.clone().requires_grad_()
        gy = torch.randn(B, cout, side, side, generator=g).to(DEV).to(dtype)

        def step(f):
            return lambda: f().backward(gy)
        if r <= 256:
            paths["fused"] = step(lambda: HF.conv1x1_chain(xg, wi, wo, bb))
        paths["two"] = step(lambda: HF.pointwise(HF.pointwise(xg, wi, None, "tadmm_tucker_1x1"), wo, bb, "tadmm_tucker_1x1"))
        paths["ref"] = step(lambda: F.conv2d(F.conv2d(xg, wic[:, :, None, None]), woc[:, :, None, None], bc))
        paths["dense"] = step(lambda: F.conv2d(xg, wd, bc))
        ctx = torch.enable_grad()
    with ctx:
        t = measure(paths, iters, rounds)
    es = x.element_size()
    io_bytes = B * side * side * (cin + cout) * es
    mid = B * side * side * r * es * 2
    row = dict(table=table, layer=name, B=B, cin=cin, cout=cout, r=r, hw=side * side, dtype=str(dtype)[6:],
               mode="fwd+bwd" if train else "inference")
    for p, (med, lo, hi) in t.items():
        row[p + "_ms"] = round(med, 4)
        row[p + "_spread"] = [round(lo, 4), round(hi, 4)]
    if not train:
        for p in t:
            byts = io_bytes + (mid if p in ("two", "ref") else 0)
            row[p + "_bw_share"] = round(byts / HBM_BPS * 1e3 / t[p][0], 3)
    if "fused" in t:
        row["two_over_fused"] = round(t["two"][0] / t["fused"][0], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="inference only, fewer rounds")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    iters, rounds = (10, 3) if a.quick else (20, 5)
    rows = []
    for table, name, B, cin, cout, r, side in layers():
        for dtype in (torch.float32, torch.bfloat16):
            for train in ((False,) if a.quick else (False, True)):
                row = bench_layer(table, name, B, cin, cout, r, side, dtype, train, iters, rounds)
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
