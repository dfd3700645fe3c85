"""A training step through the factorised convolution y = W3 conv_kxk(W1 x; Wc) + b at the shapes of the layer tables: the
3 x 3 cores of resnet18_tt 2x, resnet50_tt 3x, tk_resnet50 3x (batch 32, ImageNet planes) and tk_resnet32 3x (batch 128,
CIFAR planes) that the one-launch kernel takes (`ops.conv_chain_fits`), fp32 and bf16, forward + backward.

Classes: frozen   -- only x wants a gradient (a compressed layer that passes a gradient on): nothing is saved
         training -- W1, Wc, W3 and the bias want gradients too: the launches store H1 / H2 and dH1 / dH2
Paths:   old      -- what the layers run in grad mode without this path: `HF.pointwise` (1x1), the device library's
                     conv2d, `HF.pointwise` (1x1 + bias), three launches forward and three data-gradient launches: the
                     yardstick, timed in the same process
         new      -- `HF.conv_chain`: one launch forward, one for the data gradient (three where `ops.conv_chain_bwd_fits`
                     is False); training: dWc through the device library's weight gradient
         new_nat  -- training only: the same with dWc through `ops.core_conv_wgrad`
Timing: HIP events around ITERS calls after a warm-up, ROUNDS rounds with the order of the paths rotated every round; the
median and the spread (min..max) of the rounds are reported.  `ahead` is true when the new median is below the old
path's fastest round -- the one criterion of `ops.conv_chain_train_pays`.

    python scripts/bench_conv_train.py [--quick] [--json OUT]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "dnn-compression-tensor-admm_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_core_conv import TABLES, geometry, measure  # noqa: E402
from tadmm import functional as HF  # noqa: E402
from tadmm import hp, ops, workloads  # noqa: E402

DEV = torch.device("cuda", 0)


def shapes():
    """(table, layer, batch, C, O, r1, r2, side, k, stride) of the distinct 3 x 3 layers."""
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
            sig = (batch, shp[1], shp[0], r1, r2, side, shp[2], stride)
            if sig not in seen:
                seen.add(sig)
                out.append((key.split("_hp")[0], name) + sig)
    return out


def bench_shape(table, name, B, C, O, r1, r2, side, k, stride, dtype, training, iters, rounds):
    g = torch.Generator().manual_seed(0)
    pad = k // 2
    x = torch.randn(B, C, side, side, generator=g).to(DEV).to(dtype).requires_grad_()
    w1 = (torch.randn(r1, C, generator=g) * C ** -0.5).to(DEV).requires_grad_(training)
    core = (torch.randn(r2, r1, k, k, generator=g) * (r1 * k * k) ** -0.5).to(DEV).requires_grad_(training)
    w3 = (torch.randn(O, r2, generator=g) * r2 ** -0.5).to(DEV).requires_grad_(training)
    bias = torch.randn(O, generator=g).to(DEV).requires_grad_(training)
    side_o = (side + 2 * pad - k) // stride + 1
    gy = torch.randn(B, O, side_o, side_o, generator=g).to(DEV).to(dtype)
    n = HF._nplanes(x)
    # frozen factors: both paths reuse packed planes, as a layer's inference caches would
    p1 = None if training else HF.planes_of(w1, n)
    p3 = None if training else HF.planes_of(w3, n)
    cache = None if training else {}

    def old():
        h1 = HF.pointwise(x, w1, None, "tadmm_tucker_1x1", p1)
        h2 = F.conv2d(h1, core if dtype == core.dtype else core.to(dtype), None, stride, pad)
        HF.pointwise(h2, w3, bias, "tadmm_tucker_1x1", p3).backward(gy)

    def new(native):
        def run():
            HF.CONV_CHAIN_DWC_NATIVE = native
            HF.conv_chain(x, w1, core, w3, bias, stride, pad, 1, cache=cache).backward(gy)
        return run

    paths = {"old": old, "new": new(False)}
    if training:
        paths["new_nat"] = new(True)
    keep = HF.CONV_CHAIN_DWC_NATIVE
    try:
        t = measure(paths, iters, rounds)
    finally:
        HF.CONV_CHAIN_DWC_NATIVE = keep
    geom = ((k, k), (stride, stride), (pad, pad), (1, 1))
    fplan = ops._conv_chain_plan(x, r1, r2, *geom)
    row = dict(table=table, layer=name, B=B, C=C, O=O, r1=r1, r2=r2, side=side, k=k, stride=stride, dtype=str(dtype)[6:],
               cls="training" if training else "frozen", tiles_fwd=fplan[3], bwd_fits=ops.conv_chain_bwd_fits(x, r1, r2, *geom))
    for p, (med, lo, hi) in t.items():
        row[p + "_ms"] = round(med, 4)
        row[p + "_spread"] = [round(lo, 4), round(hi, 4)]
    for p in paths:
        if p != "old":
            row["old_over_" + p] = round(t["old"][0] / t[p][0], 3)
            row["ahead_" + p] = bool(t[p][0] < t["old"][1])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer iterations and rounds")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    iters, rounds = (5, 3) if a.quick else (20, 5)
    rows = []
    for table, name, B, C, O, r1, r2, side, k, stride in shapes():
        for dtype in (torch.float32, torch.bfloat16):
            probe = torch.empty(B, C, side, side, dtype=dtype, device="meta")
            if not ops.conv_chain_fits(probe, r1, r2, (k, k), (stride, stride), (k // 2, k // 2), (1, 1)):
                continue
            for training in (False, True):
                row = bench_shape(table, name, B, C, O, r1, r2, side, k, stride, dtype, training, iters, rounds)
                rows.append(row)
                print(json.dumps(row), flush=True)
    for cls in ("frozen", "training"):
        for dt in ("float32", "bfloat16"):
            sel = [r for r in rows if r["cls"] == cls and r["dtype"] == dt]
            for p in ("new", "new_nat"):
                if sel and ("ahead_" + p) in sel[0]:
                    ratios = sorted(r["old_over_" + p] for r in sel)
                    print(f"# {cls} {dt} {p}: ahead at {sum(r['ahead_' + p] for r in sel)} of {len(sel)}, old/new "
                          f"{ratios[0]} .. {ratios[-1]}", flush=True)
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
