"""One Riemannian SGD step (momentum 0.9) over the 60 Stiefel factors of `tk_resnet32_hp.HyperParamsDictRatio3x` -- the
two factor matrices (in_channels x in_rank, out_channels x out_rank) of each of the 30 Tucker-2 convolutions of
stftkc_resnet32 (shapes from tadmm/workloads.py).

Paths:   native   -- `ops.StiefelPlan.step`: ONE launch of csrc/stiefel.hip for all 60 factors
         composed -- the same plan with `native=False`: per factor, a few float64 library calls on the device (products,
                     `torch.linalg.cholesky_ex`, `solve_triangular`), the route of the factors that do not fit the LDS.
                     It is the only comparator there is: geoopt is not installed.
Timing: HIP events around ITERS calls after a warm-up, ROUNDS rounds with the order of the paths rotated every round; the
median and the spread (min..max) of the rounds are reported.  `ahead` is true when the native median is below the composed
route's fastest round.

`--adam` measures one Riemannian Adam step (`ops.StiefelPlan.adam_step`, betas (0.9, 0.999), eps 1e-8) over the same 60
factors instead: native (one launch of the Adam instantiation), composed (`native=False`), and the native SGD step with
momentum 0.9 in the same process as the yardstick; `adam_minus_sgd_ms` is the difference of the two native medians.

    python scripts/bench_stiefel.py [--adam] [--quick] [--json OUT]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "dnn-compression-tensor-admm_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_core_conv import measure  # noqa: E402
from tadmm import hp, ops, workloads  # noqa: E402

DEV = torch.device("cuda", 0)
KEY = "tk_resnet32_hp.HyperParamsDictRatio3x"


def factor_shapes():
    table = hp.fresh_table(KEY)
    fn = workloads.shape_fn_for(KEY)
    out = []
    for name, ranks in table.ranks.items():
        shp = fn(name)
        if len(shp) == 4 and not isinstance(ranks, int) and len(ranks) == 2:
            # (layer2.0.conv1 lists in_rank 20 for 16 input channels: StfTKConv2dC clamps a rank to its channel count)
            out.append((shp[1], min(ranks[1], shp[1])))      # first_kernel (in_channels, in_rank)
            out.append((shp[0], min(ranks[0], shp[0])))      # last_kernel (out_channels, out_rank)
    return out


def factors(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    fac = []
    for n, p in shapes:
        x = torch.linalg.qr(torch.randn(n, p, generator=g))[0].contiguous().to(DEV)
        grad = (torch.randn(n, p, generator=g) / (n * p) ** 0.5).to(DEV)
        fac.append((x, grad, torch.zeros(n, p, device=DEV)))
    return fac


def adam_state(n):
    return (torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV))


def main_adam(a, shapes, iters, rounds):
    native = ops.StiefelPlan(factors(shapes, 0))
    composed = ops.StiefelPlan(factors(shapes, 0), native=False)
    sgd = ops.StiefelPlan(factors(shapes, 0))
    sn, sc = adam_state(len(shapes)), adam_state(len(shapes))
    hyper = (0.01, (0.9, 0.999), 1e-8, 0.0, False)
    paths = {"native": lambda: native.adam_step(*hyper, *sn), "composed": lambda: composed.adam_step(*hyper, *sc),
             "native_sgd": lambda: sgd.step(0.01, 0.9)}
    t = measure(paths, iters, rounds)
    assert native.failed() == [] and composed.failed() == [] and sgd.failed() == []
    assert torch.equal(sn[2], sc[2])                                      # both routes counted the same steps
    worst = max(float((x[0] - y[0]).abs().max()) for x, y in zip(native.factors, composed.factors))
    # the project's rule: ahead by more than the min..max spread of both
    gap = t["composed"][0] - t["native"][0]
    spread = (t["native"][2] - t["native"][1]) + (t["composed"][2] - t["composed"][1])
    row = {"table": KEY, "factors": len(shapes), "optimiser": "adam", "native_ms": t["native"], "composed_ms": t["composed"],
           "native_sgd_ms": t["native_sgd"], "adam_minus_sgd_ms": t["native"][0] - t["native_sgd"][0],
           "ahead": gap > spread, "max_abs_difference_after_the_timed_steps": worst}
    print(f"{len(shapes)} factors of {KEY}, one Adam step (betas (0.9, 0.999)); SGD with momentum 0.9 as the yardstick")
    for n in ("native", "composed", "native_sgd"):
        med, lo, hi = t[n]
        print(f"  {n:10s} {med:9.4f} ms  ({lo:.4f}..{hi:.4f})")
    print(f"  native Adam - native SGD: {row['adam_minus_sgd_ms']:.4f} ms   ahead of composed by more than both spreads: "
          f"{row['ahead']}   max |X_native - X_composed| after the timed steps: {worst:.3e}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer iterations and rounds")
    ap.add_argument("--json", default=None)
    ap.add_argument("--adam", action="store_true", help="the Adam step, with the native SGD step as the yardstick")
    a = ap.parse_args()
    iters, rounds = (5, 3) if a.quick else (20, 5)
    shapes = factor_shapes()
    assert all(ops.stiefel_fits(n, p) for n, p in shapes)
    if a.adam:
        return main_adam(a, shapes, iters, rounds)
    native = ops.StiefelPlan(factors(shapes, 0))
    composed = ops.StiefelPlan(factors(shapes, 0), native=False)
    paths = {"native": lambda: native.step(0.01, 0.9), "composed": lambda: composed.step(0.01, 0.9)}
    t = measure(paths, iters, rounds)
    assert native.failed() == [] and composed.failed() == []
    worst = max(float((a[0] - b[0]).abs().max()) for a, b in zip(native.factors, composed.factors))
    row = {"table": KEY, "factors": len(shapes), "rows_max": max(n for n, _ in shapes), "cols_max": max(p for _, p in shapes),
           "native_ms": t["native"], "composed_ms": t["composed"], "ahead": t["native"][0] < t["composed"][1],
           "max_abs_difference_after_the_timed_steps": worst}
    print(f"{len(shapes)} factors of {KEY} (up to {row['rows_max']} x {row['cols_max']}), one step, momentum 0.9")
    for n in ("native", "composed"):
        med, lo, hi = t[n]
        print(f"  {n:9s} {med:9.4f} ms  ({lo:.4f}..{hi:.4f})")
    print(f"  ahead: {row['ahead']}   max |X_native - X_composed| after the timed steps: {worst:.3e}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
