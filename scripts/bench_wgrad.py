"""Weight-gradient products of the factorised layers at the shapes of their tables: dWin = (Wout^T dY)^T X (rank x in) and
dWout = dY^T (Win X) (out x rank) of the 28 single-rank layers of svd_mobilenetv2_cifar 2x at batch 128, those of
tk_resnet50 3x at batch 64 (NCHW images), and of DeiT-S qkv / proj / fc1 / fc2 at 64 x 197 tokens (token rows, the middle
TT rank of the table), fp32 and bf16.

Variants:  wgrad    -- ops.wgrad on the operands in place (csrc/wgrad.hip)
           parent   -- what the layers did before: fp32 channel-major copies (images) + ops.mm, copies included
           lib      -- torch.mm on channel-major operands made beforehand (the library's best case)
           lib+copy -- the same with the time of making them
Timing: HIP events around ITERS calls after a warm-up, ROUNDS rounds with the order of the variants rotated every round;
median and spread (min..max) of the rounds.  floor = (M + N) * T * sizeof / 8 TB/s: the product is bandwidth-bound for
small M, N.  `--threshold` sweeps T at a few (M, N) for the `_Mm` switch of tadmm/functional.py (wgrad vs ops.mm, rows).

    python scripts/bench_wgrad.py [--quick] [--threshold] [--json OUT]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "dnn-compression-tensor-admm_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_svd_layers import layers, measure  # noqa: E402
from tadmm import hp, ops, tt_layers  # noqa: E402

HBM_BPS = 8.0e12
DEV = torch.device("cuda", 0)


def channel_major(t):
    if t.dim() == 4:
        return t.permute(1, 0, 2, 3).reshape(t.shape[1], -1).float().contiguous()
    return t.float().t().contiguous()


def parent(a, b):
    if a.dim() == 4:
        return ops.mm(channel_major(a), channel_major(b).t())
    return ops.mm(a.float().t(), b.float())


def tile_of(m):
    """The tile rule of csrc/wgrad.hip (wgrad_tile): the largest of 64 / 32 / 16 that pads the side by at most 1/8 more
    than 16-wide tiles would."""
    p16 = -(-m // 16) * 16
    for t in (64, 32):
        if -(-m // t) * t * 8 <= p16 * 9:
            return t
    return 16


def workgroups(M, N, slices, nbytes):
    tm, tn = tile_of(M), tile_of(N)
    tiles = -(-M // tm) * -(-N // tn)
    assert slices == 1 or nbytes == slices * tiles * tm * tn * 4, "tile rule of the script and of the library differ"
    return tiles * slices


def shapes(quick):
    out = []
    for table, name, B, cin, cout, r, side in layers():
        out.append((f"{table} {name} dWin", (B, r, side, side), (B, cin, side, side)))
        out.append((f"{table} {name} dWout", (B, cout, side, side), (B, r, side, side)))
    table = hp.fresh_table("tt_deit_small_patch16_224_hp.HyperParamsDictRatio2x")
    for lname, fin, fout in (("blocks.1.attn.qkv.weight", 384, 1152), ("blocks.1.attn.proj.weight", 384, 384),
                             ("blocks.1.mlp.fc1.weight", 384, 1536), ("blocks.1.mlp.fc2.weight", 1536, 384)):
        lin = tt_layers.TTLinearM(fin, fout, bias=True, hp_dict=table, name=lname)
        r = lin.tt_ranks[lin.out_tt_order]
        out.append((f"deit_small {lname[9:-7]} dWin", (12608, r), (12608, fin)))
        out.append((f"deit_small {lname[9:-7]} dWout", (12608, fout), (12608, r)))
    return out[::7] if quick else out


def bench(name, sa, sb, dtype, iters, rounds):
    a = torch.randn(*sa, device=DEV).to(dtype)
    b = torch.randn(*sb, device=DEV).to(dtype)
    M, N = sa[1], sb[1]
    T = a.numel() // M
    nbytes, slices = ops.wgrad_plan(a, b)
    out = torch.empty(M, N, device=DEV)
    ta, tb = channel_major(a).to(dtype), channel_major(b).to(dtype)          # (M, T), (N, T) in the operands' dtype
    paths = {
        "wgrad": lambda: ops.wgrad(a, b, out=out),
        "parent": lambda: parent(a, b),
        "lib": lambda: torch.mm(ta, tb.t()),
        "lib+copy": lambda: torch.mm(channel_major(a).to(dtype), channel_major(b).to(dtype).t()),
    }
    res = measure(paths, iters, rounds)
    floor_ms = (M + N) * T * a.element_size() / HBM_BPS * 1e3
    wgs = workgroups(M, N, slices, nbytes)
    row = dict(shape=name, dtype=str(dtype)[6:], M=M, N=N, T=T, slices=slices, workgroups=wgs, workspace=nbytes,
               floor_ms=floor_ms,
               **{k: dict(ms=v[0], lo=v[1], hi=v[2]) for k, v in res.items()})
    w, p = res["wgrad"], res["parent"]
    verdict = "faster" if w[2] < p[1] else ("WITHIN SPREAD" if w[0] < p[0] else "SLOWER")
    print(f"{name:48s} {row['dtype']:8s} {M:5d}x{N:<5d} T={T:<7d} slices={slices:<4d} wgs={wgs:<4d} "
          f"wgrad {w[0]:8.4f} ({w[1]:.4f}..{w[2]:.4f})  parent {p[0]:8.4f} ({p[1]:.4f}..{p[2]:.4f})  "
          f"lib {res['lib'][0]:8.4f}  lib+copy {res['lib+copy'][0]:8.4f}  floor {floor_ms:7.4f} ms  {verdict}", flush=True)
    row["verdict"] = verdict
    return row


def threshold(iters, rounds):
    rows = []
    for M, N in ((18, 24), (40, 48), (64, 256), (256, 384)):
        for T in (64, 128, 256, 512, 1024, 2048, 4096, 12608):
            a = torch.randn(T, M, device=DEV)
            b = torch.randn(T, N, device=DEV)
            res = measure({"wgrad": lambda: ops.wgrad(a, b), "mm": lambda: ops.mm(a.t(), b)}, iters, rounds)
            w, m = [[v * 1e3 for v in res[k]] for k in ("wgrad", "mm")]
            print(f"threshold M={M:4d} N={N:4d} T={T:6d}  wgrad {w[0]:7.1f} ({w[1]:.1f}..{w[2]:.1f}) us  "
                  f"ops.mm {m[0]:7.1f} ({m[1]:.1f}..{m[2]:.1f}) us  {'wgrad ahead' if w[2] < m[1] else 'mm ahead' if m[2] < w[1] else 'overlap'}",
                  flush=True)
            rows.append(dict(M=M, N=N, T=T, wgrad_us=w, mm_us=m))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--threshold", action="store_true")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json")
    args = ap.parse_args()
    result = {}
    if args.threshold:
        result["threshold"] = threshold(20, args.rounds)
    else:
        rows = []
        for name, sa, sb in shapes(args.quick):
            for dtype in (torch.float32, torch.bfloat16):
                rows.append(bench(name, sa, sb, dtype, args.iters, args.rounds))
        bad = [r for r in rows if r["verdict"] != "faster"]
        print(f"{len(rows)} cases, wgrad faster than parent beyond the spread on {len(rows) - len(bad)}")
        for r in bad:
            print("  not faster:", r["shape"], r["dtype"], r["verdict"])
        result["rows"] = rows
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
