"""What the BertAdam tests share: the G17 fixture (tests/golden/make_golden_bertadam.py, recorded from the reference's
own BertAdam on the CPU in float32), optimisers built as the fixture's cases were, and the error metric."""
import functools
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 1e-5          # the project's bar on max|a - ref| / max|ref|


@functools.lru_cache(maxsize=None)
def fixture():
    """(index, arrays): the arrays a case shares with `main` are filled in from it.  Loaded once, never modified."""
    with open(os.path.join(GOLDEN, "g17_bertadam.json")) as f:
        index = json.load(f)
    with np.load(os.path.join(GOLDEN, "g17_bertadam.npz")) as z:
        arr = {k: z[k] for k in z.files}
    for key in index["same_as_main"]:
        arr[key] = arr["main_" + key.partition("_")[2]]
    for a in arr.values():
        a.setflags(write=False)
    return index, arr


def rel_err(a, ref) -> float:
    """max|a - ref| / max|ref| over the elements where ref is finite (all of them unless a case says otherwise)."""
    a = np.asarray(a, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    ok = np.isfinite(ref)
    if not ok.any():
        return 0.0
    scale = max(np.abs(ref[ok]).max(), 1e-30)
    return float(np.abs(a[ok] - ref[ok]).max() / scale)


def make_params(index, arr, device, dtype=torch.float32, source="init_{i}"):
    return [torch.nn.Parameter(torch.from_numpy(arr[source.format(i=i)].copy()).to(device=device, dtype=dtype))
            for i in range(len(index["shapes"]))]


def make_optimizer(cls, index, params, hyper):
    groups = [{"params": [params[i] for i in g["params"]], "weight_decay": g["weight_decay"]} for g in index["groups"]]
    return cls(groups, **hyper)


def set_grads(index, arr, params, k, case):
    """The gradients of step k (fresh tensors, as a backward pass after zero_grad() leaves them)."""
    for i, p in enumerate(params):
        g = torch.from_numpy(arr[f"grad_{k}_{i}"].copy())
        if case == "inf" and [k, i] == index["inf_at"][:2]:
            g.view(-1)[index["inf_at"][2]] = float("inf")
        p.grad = g.to(device=p.device, dtype=p.dtype)


def check_step(index, arr, opt, params, case, k, bar=BAR, report=None):
    """p, next_m, next_v and the counters after step k of `case` against the fixture: the same elements non-finite, the
    others within `bar`; returns the largest error."""
    worst = 0.0
    for i, p in enumerate(params):
        st = opt.state[p]
        assert type(st["step"]) is int and st["step"] == index["cases"][case]["step"][k][i]
        for what, t in (("p", p.detach()), ("m", st["next_m"]), ("v", st["next_v"])):
            ref = arr[f"{case}_{what}_{k}_{i}"]
            got = t.detach().double().cpu().numpy()
            assert got.shape == ref.shape
            assert np.array_equal(np.isfinite(got), np.isfinite(ref)), (case, what, k, i)
            err = rel_err(got, ref)
            worst = max(worst, err)
            if report is not None:
                report.append((case, k, i, what, err))
            assert err <= bar, (case, what, k, i, err)
    return worst
