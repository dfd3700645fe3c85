"""A training step (forward + backward, every factor and x wanting a gradient) through the fused linear chains, on the
route that saves the middle-rank intermediates against the route that recomputes them, in one process:

  TTLinearM   the four linear shapes of a DeiT-small block (qkv, proj, fc1, fc2) at 64 x 197 = 12 608 tokens: the cores
              are contracted into Win / Wout as the layer does in grad mode (`TTLinearM._factors`, differentiable), then
              `HF.linear_chain(..., save=True | False)`
  SVDConv2dC  1x1 layers of svd_mobilenetv2_cifar (batch 128) and tk_resnet50 (batch 32) at the layer's shapes through
              `HF.conv1x1_chain(..., save=True | False)`, the function the layer calls when `ops.svd_conv_pays`

Routes:  recompute -- save=False: dX by the fused launch, then two `ops.chain_single` launches rebuild dH and H for the
                      two `ops.wgrad` launches (the code before the saving entries existed: the yardstick)
         save      -- save=True: `_fwd_save` stores H, `_bwd_save` stores dH, two `ops.wgrad` launches
Timing: HIP events around ITERS steps after a warm-up, ROUNDS rounds with the order of the routes rotated every round;
median and spread (min..max) of the rounds.  `ahead` is true when the slowest round of the saved route is below the
fastest round of the other: the spreads do not overlap.  That is the one criterion of `ops.chain_train_pays`.
`extra_bytes` is what the saved route keeps alive from forward to backward that the other does not (H).

    python scripts/bench_linear_train.py [--quick] [--json OUT]
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
from tadmm import functional as HF  # noqa: E402
from tadmm import hp, ops, tt_layers  # noqa: E402

DEV = torch.device("cuda", 0)
TOKENS = 64 * 197
DEIT = "tt_deit_small_patch16_224_hp.HyperParamsDictRatio2x"
LINEAR = (("blocks.1.attn.qkv.weight", 384, 1152), ("blocks.1.attn.proj.weight", 384, 384),
          ("blocks.1.mlp.fc1.weight", 384, 1536), ("blocks.1.mlp.fc2.weight", 1536, 384))
# (table, layer, batch, C_in, side, rank, C_out)
CONV1X1 = (("svd_mobilenetv2_cifar", "bottlenecks.3.conv1", 128, 24, 16, 18, 144),
           ("tk_resnet50 3x", "layer1.x.conv3", 32, 64, 56, 32, 256),
           ("tk_resnet50 3x", "layer3.x.conv3", 32, 256, 14, 64, 1024),
           ("tk_resnet50 3x", "layer4.x.conv1", 32, 2048, 7, 96, 512))


def _row(kind, name, dtype, r, n_in, n_out, tokens, extra, t, rule):
    (sm, slo, shi), (rm, rlo, rhi) = t["save"], t["recompute"]
    return dict(kind=kind, layer=name, dtype=str(dtype)[6:], tokens=tokens, n_in=n_in, rank=r, n_out=n_out,
                recompute_ms=round(rm, 4), recompute_spread=[round(rlo, 4), round(rhi, 4)],
                save_ms=round(sm, 4), save_spread=[round(slo, 4), round(shi, 4)],
                recompute_over_save=round(rm / sm, 3), ahead=bool(shi < rlo), behind=bool(slo > rhi),
                extra_bytes=int(extra), rule=bool(rule))


def bench_linear(lname, fin, fout, dtype, iters, rounds):
    table = hp.fresh_table(DEIT)
    lin = tt_layers.TTLinearM(fin, fout, bias=True, hp_dict=table, name=lname).to(DEV)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(TOKENS, fin, generator=g).to(DEV).to(dtype).requires_grad_()
    gy = torch.randn(TOKENS, fout, generator=g).to(DEV).to(dtype)
    r = lin.tt_ranks[lin.out_tt_order]

    def step(save):
        def run():
            w_in, w_out = lin._factors()
            HF.linear_chain(x, w_in, w_out, lin.bias, save=save).backward(gy)
        return run

    t = measure({"recompute": step(False), "save": step(True)}, iters, rounds)
    epl = 16 // x.element_size()
    extra = TOKENS * (-(-r // epl) * epl) * x.element_size()
    return _row("TTLinearM", lname[:-7], dtype, r, fin, fout, TOKENS, extra, t, ops.chain_train_pays(x, r, fin, fout, False))


def bench_conv(table, lname, B, cin, side, r, cout, dtype, iters, rounds):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, cin, side, side, generator=g).to(DEV).to(dtype).requires_grad_()
    wi = (torch.randn(r, cin, generator=g) * cin ** -0.5).to(DEV).requires_grad_()
    wo = (torch.randn(cout, r, generator=g) * r ** -0.5).to(DEV).requires_grad_()
    b = torch.randn(cout, generator=g).to(DEV).requires_grad_()
    gy = torch.randn(B, cout, side, side, generator=g).to(DEV).to(dtype)

    def step(save):
        return lambda: HF.conv1x1_chain(x, wi, wo, b, save=save).backward(gy)

    t = measure({"recompute": step(False), "save": step(True)}, iters, rounds)
    extra = B * r * side * side * x.element_size()
    return _row("SVDConv2dC", f"{table} {lname}", dtype, r, cin, cout, B * side * side, extra, t,
                ops.chain_train_pays(x, r, cin, cout, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer iterations and rounds")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    iters, rounds = (5, 3) if a.quick else (20, 7)
    rows = []
    for dtype in (torch.float32, torch.bfloat16):
        for lname, fin, fout in LINEAR:
            rows.append(bench_linear(lname, fin, fout, dtype, iters, rounds))
            print(json.dumps(rows[-1]), flush=True)
        for case in CONV1X1:
            rows.append(bench_conv(*case, dtype, iters, rounds))
            print(json.dumps(rows[-1]), flush=True)
    for kind in ("TTLinearM", "SVDConv2dC"):
        for dt in ("float32", "bfloat16"):
            sel = [r for r in rows if r["kind"] == kind and r["dtype"] == dt]
            ratios = sorted(r["recompute_over_save"] for r in sel)
            print(f"# {kind} {dt}: saved route ahead beyond the spread at {sum(r['ahead'] for r in sel)} of {len(sel)}, "
                  f"behind at {sum(r['behind'] for r in sel)}, recompute/save {ratios[0]} .. {ratios[-1]}", flush=True)
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
