"""float16 inference of the TT layers against bfloat16, the float32 per-core route and the dense layer.

Rows: the four TTLinearM shapes of a DeiT-small block at 64 x 197 = 12 608 tokens and one TTConv2dM 3x3 layer of every
ResNet-18 stage at batch 64, all under `torch.no_grad()`.
Paths:  f16    -- layer(x.half()): the one-plane kernels with the f16 MFMA (or what `ops` routes float16 to)
        bf16   -- layer(x.bfloat16()): the existing path
        chain  -- the route a float16 input took before float16 reached the kernels: the per-core chain through the fp32
                  GEMM (`TTLinearM._forward_chain` / `TTConv2dM._chains`, float32 copies of every operand, float32 result).
                  Those two methods are the code the earlier forward called for float16, so they are timed in this
                  process rather than from a second build
        dense  -- F.linear / F.conv2d in float16 on the device library with the recovered dense weight
        three  -- (convolutions) the layer's other native route in float16: `tadmm_ttconv_chain_in`, the device library's
                  k x k conv2d, `tadmm_ttconv_chain_out` -- what `ops.conv_chain_pays` chooses between
        dense_bf16 -- (convolutions) the dense layer in bfloat16, to tell a float16 matter from one both types share
Timing: HIP events around ITERS calls after a warm-up, ROUNDS rounds with the order of the paths rotated every round;
median and min..max of the rounds.

    python scripts/bench_fp16_forward.py [--quick] [--json OUT]
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
from tadmm import hp as HPM  # noqa: E402
from tadmm import ops, tt_layers  # noqa: E402

DEV = torch.device("cuda", 0)


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


def row_of(name, t, extra):
    row = dict(layer=name, **extra)
    for p, (med, lo, hi) in t.items():
        row[p + "_ms"] = round(med, 4)
        row[p + "_spread"] = [round(lo, 4), round(hi, 4)]
    for p in t:
        if p != "f16":
            row[p + "_over_f16"] = round(t[p][0] / t["f16"][0], 3)
    # "loses": slower than the other path by more than the min..max spread of both rows
    row["f16_loses_to"] = [p for p in t if p not in ("f16", "bf16", "dense_bf16") and t["f16"][1] > t[p][2]]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer iterations and rounds")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    iters, rounds = (10, 3) if a.quick else (30, 5)
    g = torch.Generator().manual_seed(0)
    rows = []
    with torch.no_grad():
        hp = HPM.fresh_table("tt_deit_small_patch16_224_hp.HyperParamsDictRatio2x")
        for lname, fin, fout in (("blocks.1.attn.qkv.weight", 384, 1152), ("blocks.1.attn.proj.weight", 384, 384),
                                 ("blocks.1.mlp.fc1.weight", 384, 1536), ("blocks.1.mlp.fc2.weight", 1536, 384)):
            if lname not in hp.tt_shapes:
                continue
            lin = tt_layers.TTLinearM(fin, fout, bias=True, hp_dict=hp, name=lname).to(DEV)
            w_in, w_out = lin._factors()
            wd, bd = (w_out @ w_in).half().contiguous(), lin.bias.detach().half()
            x = torch.randn(64, 197, fin, generator=g).to(DEV)
            xh, xb = x.half(), x.bfloat16()
            rq = lin.tt_ranks[lin.out_tt_order]
            t = measure({"f16": lambda: lin(xh), "bf16": lambda: lin(xb), "chain": lambda: lin._forward_chain(xh),
                         "dense": lambda: F.linear(xh, wd, bd)}, iters, rounds)
            route = "dense weight" if lin._dense_pays(xh, rq) else ("fused chain" if lin._fused_ok(xh) else "per-core chain")
            rows.append(row_of("TTLinearM deit_small " + lname[:-7], t, dict(tokens=64 * 197, fin=fin, fout=fout, rank=rq,
                                                                             f16_route=route)))
            print(json.dumps(rows[-1]), flush=True)
        hp18 = HPM.fresh_table("tt_resnet18_hp.HyperParamsDictGeneralRatio2x")
        for lname, ch, hw in (("layer1.1.conv1.weight", 64, 56), ("layer2.1.conv1.weight", 128, 28),
                              ("layer3.1.conv1.weight", 256, 14), ("layer4.0.conv2.weight", 512, 7)):
            if lname not in hp18.tt_shapes:
                continue
            conv = tt_layers.TTConv2dM(ch, ch, 3, padding=1, bias=False, hp_dict=hp18, name=lname).to(DEV)
            w_in, w_out = conv._factors()                  # the dense kernel the three factors compose to
            wc = torch.einsum("or,rskl,sc->ockl", w_out, conv.core_kernel.detach(), w_in).half().contiguous()
            x = torch.randn(64, ch, hw, hw, generator=g).to(DEV)
            xh, xb = x.half(), x.bfloat16()
            wcb, coreh = wc.bfloat16(), conv.core_kernel.detach().half()
            p_in, p_out = HF.planes_of(w_in, 1, like=xh), HF.planes_of(w_out, 1, like=xh)

            def three():
                h1 = HF.pointwise(xh, w_in, None, "tadmm_ttconv_chain_in", p_in)
                return HF.pointwise(F.conv2d(h1, coreh, None, 1, 1), w_out, None, "tadmm_ttconv_chain_out", p_out)
            t = measure({"f16": lambda: conv(xh), "bf16": lambda: conv(xb), "chain": lambda: conv._chains(xh)[0],
                         "dense": lambda: F.conv2d(xh, wc, None, 1, 1), "three": three,
                         "dense_bf16": lambda: F.conv2d(xb, wcb, None, 1, 1)}, iters, rounds)
            one = ops.conv_chain_pays(xh, conv.in_tt_ranks[0], conv.out_tt_ranks[-1], conv.kernel_size, conv.stride,
                                      conv.padding, conv.dilation)
            rows.append(row_of("TTConv2dM resnet18 " + lname[:-7], t, dict(B=64, ch=ch, hw=hw, ranks=list(conv.tt_ranks),
                                                                           f16_route="one launch" if one else "three launches")))
            print(json.dumps(rows[-1]), flush=True)
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
