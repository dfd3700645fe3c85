"""Generate golden vectors G17 (BertAdam and its schedules) from the REAL reference.

    python tests/golden/make_golden_bertadam.py <path of the reference checkout>

Runs only where the reference is at hand.  Loads its xcompression/transformer/optimization.py as a module object and
runs the reference's OWN `BertAdam` on the CPU in float32 (it runs under a current torch with a deprecation warning
only).  Five tensors (numel 1, 3, 5, 257, 600) in two param groups (weight_decay 0.01 and 0) take 5 steps with gradients
whose norm alternates between far above and far below max_grad_norm.  All cases share the initial tensors and the
gradients (stored once); a case records p, next_m, next_v, the step counters and get_lr() after every step (an array
that equals the one of `main` bit for bit is listed under "same_as_main" instead of being stored again):
    main      warmup_linear, warmup 0.3, t_total 8: crosses the warm-up edge
    beyond    t_total 3: runs beyond it, the multiplier ends at 0
    noclip    max_grad_norm -1
    nosched   schedule 'none'
    inf       main with one inf gradient element in step 1
Also recorded: every schedule class's multiplier on a grid of progress values, and the reference optimiser's
state_dict() after 3 steps of `main`, as arrays.  The reference never travels with the tests; these data files do.
"""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

SHAPES = [(257,), (20, 30), (1,), (3,), (5,)]
GROUPS = [{"params": [0, 1, 2], "weight_decay": 0.01}, {"params": [3, 4], "weight_decay": 0.0}]
STEPS = 5
BASE = dict(lr=1e-2, warmup=0.3, t_total=8, schedule="warmup_linear", b1=0.9, b2=0.999, e=1e-6, max_grad_norm=1.0)
CASES = {
    "main": {},
    "beyond": {"t_total": 3},
    "noclip": {"max_grad_norm": -1},
    "nosched": {"schedule": "none"},
    "inf": {},
}
INF_AT = (1, 1, 17)          # (step, tensor, flat element) of the inf of case `inf`
STATE_AFTER = 3
# (class name, constructor arguments): multipliers at step / t_total for step 0 .. 60 with t_total 40
SCHEDULE_GRID = [("ConstantLR", {"warmup": 0.1}), ("WarmupConstantSchedule", {"warmup": 0.1}),
                 ("WarmupLinearSchedule", {"warmup": 0.1}), ("WarmupLinearSchedule", {"warmup": -1}),
                 ("WarmupCosineSchedule", {"warmup": 0.1}), ("WarmupCosineSchedule", {"warmup": 0.2, "cycles": 1.5}),
                 ("WarmupCosineWithHardRestartsSchedule", {"warmup": 0.1, "cycles": 3.0}),
                 ("WarmupCosineWithWarmupRestartsSchedule", {"warmup": 0.05, "cycles": 3.0})]
GRID_T_TOTAL, GRID_STEPS = 40, 61


def load(path):
    spec = importlib.util.spec_from_file_location(
        "ref_optimization", os.path.join(path, "xcompression", "transformer", "optimization.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs():
    g = torch.Generator().manual_seed(1700)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    grads = []
    for k in range(STEPS):
        scale = 50.0 if k % 2 == 0 else 1e-3          # norm far above / far below max_grad_norm = 1
        grads.append([scale * torch.randn(s, generator=g) for s in SHAPES])
    return init, grads


def main(path):
    mod = load(path)
    init, grads = inputs()
    rec = {f"init_{i}": t.numpy().copy() for i, t in enumerate(init)}
    for k in range(STEPS):
        for i, t in enumerate(grads[k]):
            rec[f"grad_{k}_{i}"] = t.numpy().copy()
    index = {"shapes": [list(s) for s in SHAPES], "groups": GROUPS, "steps": STEPS, "base": BASE, "cases": {},
             "inf_at": list(INF_AT), "state_after": STATE_AFTER}
    for name, over in CASES.items():
        hyper = dict(BASE, **over)
        params = [torch.nn.Parameter(t.clone()) for t in init]
        opt = mod.BertAdam([{"params": [params[i] for i in g["params"]], "weight_decay": g["weight_decay"]}
                            for g in GROUPS], **hyper)
        lrs = [opt.get_lr()]
        counters = []
        for k in range(STEPS):
            for i, p in enumerate(params):
                p.grad = grads[k][i].clone()
                if name == "inf" and (k, i) == INF_AT[:2]:
                    p.grad.view(-1)[INF_AT[2]] = float("inf")
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                opt.step()
            for i, p in enumerate(params):
                rec[f"{name}_p_{k}_{i}"] = p.detach().numpy().copy()
                rec[f"{name}_m_{k}_{i}"] = opt.state[p]["next_m"].numpy().copy()
                rec[f"{name}_v_{k}_{i}"] = opt.state[p]["next_v"].numpy().copy()
            lrs.append([float(x) for x in opt.get_lr()])
            counters.append([int(opt.state[p]["step"]) for p in params])
            if name == "main" and k + 1 == STATE_AFTER:
                sd = opt.state_dict()
                index["state_dict"] = {
                    "state_keys": sorted(int(i) for i in sd["state"]),
                    "entry_keys": sorted(sd["state"][0]),
                    "step": {str(i): int(s["step"]) for i, s in sd["state"].items()},
                    "step_is_int": all(type(s["step"]) is int for s in sd["state"].values()),
                    "param_groups": [{k2: (v if k2 != "schedule" else
                                           {"class": type(v).__name__, "warmup": v.warmup, "t_total": v.t_total})
                                      for k2, v in g.items()} for g in sd["param_groups"]],
                }
                for i, s in sd["state"].items():
                    rec[f"sd_m_{i}"] = s["next_m"].numpy().copy()
                    rec[f"sd_v_{i}"] = s["next_v"].numpy().copy()
        index["cases"][name] = {"hyper": hyper, "get_lr": lrs, "step": counters}
    grid = []
    for cls, kw in SCHEDULE_GRID:
        s = getattr(mod, cls)(t_total=GRID_T_TOTAL, **kw)
        grid.append({"class": cls, "kwargs": kw, "t_total": GRID_T_TOTAL,
                     "mult": [float(s.get_lr(k, nowarn=True)) for k in range(GRID_STEPS)]})
    index["schedule_grid"] = grid
    index["schedules"] = {str(k): v.__name__ for k, v in mod.SCHEDULES.items()}
    # what a case shares bit for bit with `main` (m and v do not depend on the rate; tensors are clipped one by one) is
    # stored once: "same_as_main" lists those arrays
    same = []
    for key in list(rec):
        name, _, tail = key.partition("_")
        if name in CASES and name != "main" and rec[key].tobytes() == rec["main_" + tail].tobytes():
            same.append(key)
            del rec[key]
    index["same_as_main"] = same
    np.savez_compressed(os.path.join(HERE, "g17_bertadam.npz"), **rec)
    with open(os.path.join(HERE, "g17_bertadam.json"), "w") as f:
        json.dump(index, f, indent=1)
    print("wrote", len(rec), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
