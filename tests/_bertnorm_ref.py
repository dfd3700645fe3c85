"""Float64 restatement of csrc/bertnorm.hip, forward and backward, written from the formulas:

    s = x keep / (1 - p) + res,  mean = mean_j s,  var = mean_j (s - mean)^2,  rstd = 1 / sqrt(var + eps)
    xhat = (s - mean) rstd,  y = gamma xhat + beta
    a = g gamma,  dsum = rstd (a - mean_j a - xhat mean_j(a xhat)),  dres = dsum,  dx = dsum keep / (1 - p)
    dgamma = sum_rows g xhat,  dbeta = sum_rows g

No autograd: the gradients are the closed forms above.  Also the error scale of the device tests,
A = |gamma| (|s| + |mean|) rstd + |beta|: the running-error scale of the cancellation in s - mean."""
import json
import os

import numpy as np
import torch

F64 = torch.float64


def _f64(t):
    return t.detach().to("cpu", F64)


def restate(x, res, gamma, beta, eps=1e-12, p=0.0, keep=None, g=None):
    """dict of float64 CPU tensors: y, s, A (the shape of x), mean, rstd (the shape of x with a last dimension of 1), and
    -- when the upstream gradient g is given -- dx, dres (the shape of x), dgamma, dbeta ((hidden,))."""
    X, gam, bet = _f64(x), _f64(gamma), _f64(beta)
    kp = torch.ones_like(X) if (keep is None or p == 0.0) else (keep.detach().to("cpu") != 0).to(F64) / (1.0 - p)
    s = X * kp if res is None else X * kp + _f64(res)
    mean = s.mean(dim=-1, keepdim=True)
    d = s - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(dim=-1, keepdim=True) + eps)
    xhat = d * rstd
    out = {"y": gam * xhat + bet, "s": s, "mean": mean, "rstd": rstd,
           "A": gam.abs() * (s.abs() + mean.abs()) * rstd + bet.abs()}
    if g is None:
        return out
    G = _f64(g)
    a = G * gam
    dsum = rstd * (a - a.mean(dim=-1, keepdim=True) - xhat * (a * xhat).mean(dim=-1, keepdim=True))
    hidden = X.shape[-1]
    out.update(dres=dsum, dx=dsum * kp, dgamma=(G * xhat).reshape(-1, hidden).sum(0), dbeta=G.reshape(-1, hidden).sum(0))
    return out


def golden(golden_dir):
    with open(os.path.join(golden_dir, "g19_bertnorm.json")) as f:
        return json.load(f)


def golden_index(golden_dir):
    return golden(golden_dir)["cases"]


def recorded(golden_dir, meta):
    """The arrays of one recorded case as float32 torch tensors: x, g, weight, bias, y, dx, dweight, dbias, and for the
    two sub-layer modules res and dres.  Inputs are stored as int8 numerators over 64, and dres once with dx where the
    reference returned one array for both."""
    with np.load(os.path.join(golden_dir, "g19_bertnorm.npz")) as z:
        pre = meta["name"] + "/"
        d = {}
        for key in z.files:
            if not key.startswith(pre):
                continue
            name = key[len(pre):]
            if name.endswith(".q6"):
                d[name[:-3]] = torch.from_numpy(z[key].astype(np.float32) / 64.0)
            else:
                d[name] = torch.from_numpy(z[key].copy())
    if meta["dres_is_dx"]:
        d["dres"] = d["dx"].clone()
    return d
