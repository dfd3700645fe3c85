"""LSTM recurrence: the one-launch route (csrc/lstm.hip) against the composed step loop, forward and training step.

    python scripts/bench_lstm.py [--repeats 7] [--iters 10] [--layer]

The yardstick is the step loop below, written from operations the library had before the launch existed
(`functional.mm`, torch pointwise), so this file runs unchanged on a checkout without the launch and then times the
yardstick alone.  The recurrence depends on (T, B, H) only: UCF11 and YTC share H = 256 (compare_tt_lstm.py:42-50), TIMIT's
H = 512 is beyond the launch and is timed on the composed loop alone; H = 64 and 128 widen the routing rule.  `--layer`
adds the whole TTLSTM layer (TT input map + recurrence) at the three datasets' shapes.

Every figure: median of `--repeats` windows of `--iters` calls each, host clock around work that ends in a device
synchronise, after 3 warm-up calls per shape; min..max of the windows is the spread.  `ahead` is printed only when the
launch's max is below the yardstick's min (or the other way round), the rule every `*_pays` function follows.
"""
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

DEV = "cuda:0"
DATASETS = {   # name: (in_tt, out_tt, ranks)   compare_tt_lstm.py:42-55
    "ucf11": ([8, 20, 20, 18], [4, 8, 8], [1, 4, 8, 16, 8, 4, 4, 1]),
    "ytc": ([4, 20, 20, 36], [8, 8, 4], [1, 4, 8, 16, 8, 8, 4, 1]),
    "timit": ([5, 7, 9], [4, 8, 16], [1, 2, 2, 4, 2, 2, 1]),
}


def yardstick(xp, w_hh, h, c):
    """tt_lstm_inference.py:61-77 per step: one product and the pointwise gate arithmetic."""
    H = w_hh.shape[1]
    wt = w_hh.t()
    ys = []
    for t in range(xp.shape[0]):
        z = xp[t] + HF.mm(h, wt)
        i = torch.nn.functional.hardsigmoid(z[:, :H])
        f = torch.nn.functional.hardsigmoid(z[:, H:2 * H])
        o = torch.nn.functional.hardsigmoid(z[:, 3 * H:])
        c = f * c + i * torch.tanh(z[:, 2 * H:3 * H])
        h = o * torch.tanh(c)
        ys.append(h)
    return torch.stack(ys), (h, c)


def windows(fn, repeats, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters * 1e3)
    return out


def summary(ws):
    return {"median_ms": statistics.median(ws), "min_ms": min(ws), "max_ms": max(ws)}


def verdict(a, b):
    """'launch' / 'composed' when one is ahead beyond the spread of both, else 'level'."""
    if a["max_ms"] < b["min_ms"]:
        return "launch"
    if b["max_ms"] < a["min_ms"]:
        return "composed"
    return "level"


def recurrence(T, B, H, grad, repeats, iters):
    g = torch.Generator(device=DEV).manual_seed(T * 1000 + B + H)
    xp = 1.5 * torch.randn(T, B, 4 * H, device=DEV, generator=g)
    w = (torch.rand(4 * H, H, device=DEV, generator=g) * 2 - 1) * (2 / H ** 0.5)
    h0, c0 = 0.5 * torch.randn(B, H, device=DEV, generator=g), 0.5 * torch.randn(B, H, device=DEV, generator=g)
    dy = torch.randn(T, B, H, device=DEV, generator=g)
    if grad:
        xp.requires_grad_(True)
        w.requires_grad_(True)

    def call(route_fn):
        def fn():
            if not grad:
                with torch.no_grad():
                    return route_fn(xp, w, h0, c0)
            xp.grad = w.grad = None
            y, _ = route_fn(xp, w, h0, c0)
            (y * dy).sum().backward()
        return fn

    row = {"what": "train" if grad else "forward", "T": T, "B": B, "H": H}
    row["composed"] = summary(windows(call(yardstick), repeats, iters))
    launch = getattr(HF, "lstm_sequence", None)
    from tadmm import ops
    if launch is not None and ops.lstm_fits(H):
        row["launch"] = summary(windows(call(lambda *a: launch(*a, route="launch")), repeats, iters))
        # the two routes must compute the same thing at the sizes timed
        with torch.no_grad():
            ya, yb = launch(xp, w, h0, c0, route="launch")[0], yardstick(xp, w, h0, c0)[0]
        row["max_abs_diff"] = float((ya - yb).abs().max())
        row["ahead"] = verdict(row["launch"], row["composed"])
        row["speedup"] = row["composed"]["median_ms"] / row["launch"]["median_ms"]
    return row


def layer(name, T, B, grad, repeats, iters):
    from tadmm.rnn_layers import TTLSTM, entry
    in_tt, out_tt, ranks = DATASETS[name]
    n_in, H = 1, 1
    for v in in_tt:
        n_in *= v
    for v in out_tt:
        H *= v
    torch.manual_seed(1)
    m = TTLSTM(n_in, H, hp_dict=entry("rnn", [4 * out_tt[0]] + out_tt[1:] + in_tt, ranks), name="rnn").to(DEV)
    x = torch.randn(T, B, n_in, device=DEV)

    def fn():
        if not grad:
            with torch.no_grad():
                return m(x)
        m.zero_grad(set_to_none=True)
        m(x)[0].square().sum().backward()

    return {"what": "layer-train" if grad else "layer-forward", "dataset": name, "T": T, "B": B, "H": H,
            "route": summary(windows(fn, repeats, iters))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--layer", action="store_true")
    ap.add_argument("--hidden", type=int, nargs="*", default=[256, 128, 64, 512])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lstm.py needs the MI355X: a timing taken elsewhere says nothing")
    for H in a.hidden:
        for T in (6, 64):
            for B in (1, 16, 64, 256):
                for grad in (False, True):
                    print(json.dumps(recurrence(T, B, H, grad, a.repeats, a.iters if T == 6 else max(2, a.iters // 3))), flush=True)
    if a.layer:
        for name in DATASETS:
            for grad in (False, True):
                print(json.dumps(layer(name, 6, 16, grad, a.repeats, a.iters)), flush=True)


if __name__ == "__main__":
    main()
