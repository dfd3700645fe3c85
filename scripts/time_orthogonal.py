"""Time the orthogonality regulariser (orthogonal.py: append_double_l2_loss) forward + backward on five factorised
models: the fused native call against the reference's per-factor torch formulation on the same device.

HIP events around each step, medians over rounds, the order of the two variants rotated between rounds.  One JSON line
per table.  --profile N: run only N steady-state fused steps (for a kernel trace), no timing."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dnn-compression-tensor-admm_amd"))
import torch  # noqa: E402

from tadmm import workloads  # noqa: E402
from tadmm.orthogonal import append_double_l2_loss, select  # noqa: E402

RHO = 1e-3


def fused(model, dev):
    loss = append_double_l2_loss(model, torch.zeros((), device=dev), RHO, dev)
    loss.backward()


def torch_loop(model, dev):
    # orthogonal.py restated per factor (torch.eye(n).to(device) included, as the reference does)
    loss = torch.zeros((), device=dev)
    for _, p, rows in select(model):
        P = torch.squeeze(p)
        if rows:
            eye = torch.eye(p.shape[0]).to(dev)
            loss = loss + 0.5 * RHO * (torch.norm(torch.mm(P, P.t()) - eye, p=2)) ** 2
        else:
            eye = torch.eye(p.shape[1]).to(dev)
            loss = loss + 0.5 * RHO * (torch.norm(torch.mm(P.t(), P) - eye, p=2)) ** 2
    loss.backward()


def time_one(fn, model, dev, steps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        for p in model.parameters():
            p.grad = None
        a.record()
        fn(model, dev)
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tables", default=",".join(workloads.ORTH_TABLES))
    ap.add_argument("--profile", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in args.tables.split(","):
        model = workloads.orth_model(name).to(dev)
        sel = select(model)
        if args.profile:
            for _ in range(args.warmup):
                fused(model, dev)
            torch.cuda.synchronize()
            for _ in range(args.profile):
                fused(model, dev)
            torch.cuda.synchronize()
            print(json.dumps({"table": name, "profiled_steps": args.profile}), flush=True)
            continue
        variants = {"fused": fused, "torch": torch_loop}
        for fn in variants.values():
            for _ in range(args.warmup):
                fn(model, dev)
        torch.cuda.synchronize()
        res = {k: [] for k in variants}
        order = list(variants)
        for r in range(args.rounds):
            for k in order[r % 2:] + order[:r % 2]:
                res[k].append(statistics.median(time_one(variants[k], model, dev, args.steps)))
        med = {k: statistics.median(v) for k, v in res.items()}
        flop = 0
        for _, p, rows in sel:
            m = p.squeeze()
            n, k = (m.shape[0], m.shape[1]) if rows else (m.shape[1], m.shape[0])
            flop += 4 * n * n * k            # Gram + E P
        print(json.dumps({"table": name, "factors": len(sel), "gflop": round(flop / 1e9, 4),
                          "fused_ms": round(med["fused"], 4), "torch_ms": round(med["torch"], 4),
                          "speedup": round(med["torch"] / med["fused"], 2),
                          "fused_rounds_ms": [round(x, 4) for x in res["fused"]],
                          "torch_rounds_ms": [round(x, 4) for x in res["torch"]]}), flush=True)


if __name__ == "__main__":
    main()
