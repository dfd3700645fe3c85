"""Float64 restatement of the self-attention of csrc/attn.hip, forward and both gradients, written from the formulas:

    scores[b,h,i,j] = (Q[b,i,h,:] . K[b,j,h,:]) / sqrt(d) + mask[b,0,0,j]
    P = softmax_j(scores),  Pd = P * keep / (1 - p)
    context[b,i,h*d:(h+1)*d] = sum_j Pd[b,h,i,j] V[b,j,h,:]
    dPd = (g_ctx V^T) keep / (1-p),  D_i = sum_j P_ij dPd_ij,  dS = g_sc + P (dPd - D)
    dQ = dS K / sqrt(d),  dK = dS^T Q / sqrt(d),  dV = Pd^T g_ctx

No autograd: the gradients are the closed forms above.  Also the error scales of the device tests: A (the sum of the
magnitudes that make up a score) and C (the same for a context element)."""
import json
import math
import os

import numpy as np
import torch

F64 = torch.float64


def heads(t, H):
    """(B, S, H*d) -> (B, H, S, d) in float64"""
    B, S, Hd = t.shape
    return t.detach().to("cpu", F64).view(B, S, H, Hd // H).permute(0, 2, 1, 3)


def unheads(t):
    """(B, H, S, d) -> (B, S, H*d)"""
    B, H, S, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, S, H * d)


def restate(q, k, v, mask, H, p=0.0, keep=None, g_ctx=None, g_sc=None):
    """dict of float64 CPU tensors: ctx (B, S, H*d), scores (B, H, S, S), lse (B, H, S), the scales A (B, H, S, S) and
    C (B, S, H*d), and -- when an upstream gradient is given -- dq, dk, dv (B, S, H*d)."""
    Q, K, V = heads(q, H), heads(k, H), heads(v, H)
    B, _, S, d = Q.shape
    rs = 1.0 / math.sqrt(d)
    m = torch.zeros(B, 1, 1, S, dtype=F64) if mask is None else mask.detach().to("cpu", F64).reshape(B, 1, 1, S)
    scores = torch.einsum("bhid,bhjd->bhij", Q, K) * rs + m
    A = torch.einsum("bhid,bhjd->bhij", Q.abs(), K.abs()) * rs + torch.where(torch.isinf(m), torch.zeros_like(m), m.abs())
    mx = scores.max(dim=-1, keepdim=True).values
    e = torch.exp(scores - mx)
    Z = e.sum(dim=-1, keepdim=True)
    P = e / Z
    lse = (mx + torch.log(Z)).squeeze(-1)
    kp = torch.ones_like(P) if (keep is None or p == 0.0) else (keep.detach().to("cpu") != 0).to(F64) / (1.0 - p)
    Pd = P * kp
    out = {"scores": scores, "lse": lse, "A": A,
           "ctx": unheads(torch.einsum("bhij,bhjd->bhid", Pd, V)),
           "C": unheads(torch.einsum("bhij,bhjd->bhid", Pd, V.abs()))}
    if g_ctx is None and g_sc is None:
        return out
    dS = torch.zeros_like(P) if g_sc is None else g_sc.detach().to("cpu", F64).clone()
    dV = torch.zeros_like(V)
    if g_ctx is not None:
        G = heads(g_ctx, H)
        dPd = torch.einsum("bhid,bhjd->bhij", G, V) * kp
        D = (P * dPd).sum(dim=-1, keepdim=True)
        dS = dS + P * (dPd - D)
        dV = torch.einsum("bhij,bhid->bhjd", Pd, G)
    out["dq"] = unheads(torch.einsum("bhij,bhjd->bhid", dS, K) * rs)
    out["dk"] = unheads(torch.einsum("bhij,bhid->bhjd", dS, Q) * rs)
    out["dv"] = unheads(dV)
    return out


def golden_index(golden_dir):
    with open(os.path.join(golden_dir, "g18_attention.json")) as f:
        return json.load(f)["cases"]


def recorded(golden_dir, name):
    """The arrays of one recorded case as float32 torch tensors (mask: None when the case has no padding)."""
    with np.load(os.path.join(golden_dir, "g18_attention.npz")) as z:
        pre = name + "/"
        d = {key[len(pre):]: torch.from_numpy(z[key].copy()) for key in z.files if key.startswith(pre)}
    return d


def padding_mask(lengths, S, fill=-10000.0, dtype=torch.float32):
    """The reference's extended attention mask (B, 1, 1, S): 0 where a token is kept, `fill` from lengths[b] on."""
    m = torch.zeros(len(lengths), 1, 1, S, dtype=dtype)
    for b, n in enumerate(lengths):
        m[b, 0, 0, n:] = fill
    return m
