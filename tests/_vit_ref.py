"""Float64 restatement of csrc/prenorm.hip and of the dense vision transformer of tadmm/vit_layers.py.

timm is not installed where these tests run, so the reference's vit_tt.py cannot be executed and nothing can be
recorded from it: this file is the yardstick.  It is written from the formulas of the issue and from timm 0.4.x's
`DropPath`, `Attention.forward`, `Mlp.forward`, `Block.forward` and `VisionTransformer.forward`:

    scale_i = path_keep[i / N] / (1 - p_path),  s = x + scale b keep / (1 - p)
    mean = mean_j s,  var = mean_j (s - mean)^2,  rstd = 1 / sqrt(var + eps),  xhat = (s - mean) rstd,  y = gamma xhat + beta
    a = g_y gamma,  ds = g_s + rstd (a - mean_j a - xhat mean_j(a xhat)),  dx = ds,  db = ds scale keep / (1 - p)
    dgamma = sum_rows g_y xhat,  dbeta = sum_rows g_y

    attention: qkv = x Wqkv^T + bqkv, split (3, H, d); softmax(q k^T d^-1/2) v; heads concatenated; proj
    block:     x = x + attn(norm1(x));  x = x + mlp(norm2(x)),  mlp = fc2(gelu(fc1(.))),  exact (erf) GELU
    model:     patch convolution, class (and distillation) token, position embedding, blocks, norm, head(s); the mean of
               both heads in eval mode

The tail (`stream`, `layer_norm`, `tail_grads`) is closed forms without autograd.  The gradients of a whole block or
model with respect to its parameters are taken by autograd over the float64 forward written here (`block`, `vit`):
closed forms for those would restate autograd itself."""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64


def f64(t):
    return t.detach().to("cpu", F64)


def stream(x, b, p=0.0, keep=None, p_path=0.0, path_keep=None, nper=1):
    """(s, scale of s, factor) as float64 (rows, C): s = x + b factor, factor = scale keep / (1 - p), and the
    elementwise error scale |x| + |b factor|."""
    X, B = f64(x).reshape(-1, x.shape[-1]), f64(b).reshape(-1, x.shape[-1])
    factor = torch.ones_like(X)
    if keep is not None and p > 0.0:
        factor = factor * (keep.detach().to("cpu").reshape(X.shape) != 0).to(F64) / (1.0 - p)
    if path_keep is not None and p_path > 0.0:
        per_row = (path_keep.detach().to("cpu") != 0).to(F64).repeat_interleave(nper) / (1.0 - p_path)
        factor = factor * per_row[:, None]
    return X + B * factor, X.abs() + (B * factor).abs(), factor


def layer_norm(s, gamma, beta, eps=1e-6):
    """dict of float64 tensors for the LayerNorm of the rows of s: y, xhat, mean, rstd and the error scale
    A = |gamma| (|s| + |mean|) rstd + |beta| (the running-error scale of the cancellation in s - mean)."""
    S, gam, bet = f64(s).reshape(-1, s.shape[-1]), f64(gamma), f64(beta)
    mean = S.mean(dim=-1, keepdim=True)
    d = S - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(dim=-1, keepdim=True) + eps)
    xhat = d * rstd
    return {"y": gam * xhat + bet, "xhat": xhat, "mean": mean, "rstd": rstd,
            "A": gam.abs() * (S.abs() + mean.abs()) * rstd + bet.abs()}

def tail_grads(s, gamma, factor, g_y=None, g_s=None, eps=1e-6):
    """dict dx, db (rows, C), dgamma, dbeta (C,) in float64 from the closed forms; a missing gradient is zero."""
    S, gam = f64(s).reshape(-1, s.shape[-1]), f64(gamma)
    ln = layer_norm(S, gam, torch.zeros_like(gam), eps)
    xhat, rstd = ln["xhat"], ln["rstd"]
    Gy = torch.zeros_like(S) if g_y is None else f64(g_y).reshape(S.shape)
    Gs = torch.zeros_like(S) if g_s is None else f64(g_s).reshape(S.shape)
    a = Gy * gam
    ds = Gs + rstd * (a - a.mean(dim=-1, keepdim=True) - xhat * (a * xhat).mean(dim=-1, keepdim=True))
    return {"dx": ds, "db": ds * factor, "dgamma": (Gy * xhat).sum(0), "dbeta": Gy.sum(0)}


def plain_layer_norm(x, w, b, eps=1e-6):
    mean = x.mean(dim=-1, keepdim=True)
    d = x - mean
    return w * d / torch.sqrt((d * d).mean(dim=-1, keepdim=True) + eps) + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def attention(x, sd, pre, heads):
    """timm's Attention.forward in eval mode; sd[pre + 'qkv.weight'] etc. are float64 tensors."""
    B, N, C = x.shape
    d = C // heads
    qkv = x @ sd[pre + "qkv.weight"].t()
    if pre + "qkv.bias" in sd:
        qkv = qkv + sd[pre + "qkv.bias"]
    q, k, v = qkv.reshape(B, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    attn = torch.softmax((q @ k.transpose(-2, -1)) * d ** -0.5, dim=-1)
    out = (attn @ v).transpose(1, 2).reshape(B, N, C)
    return out @ sd[pre + "proj.weight"].t() + sd[pre + "proj.bias"]


def block(x, sd, pre, heads, eps=1e-6):
    """timm's Block.forward in eval mode over the float64 state dict `sd` with keys pre + 'norm1.weight' ..."""
    h = plain_layer_norm(x, sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], eps)
    x = x + attention(h, sd, pre + "attn.", heads)
    h = plain_layer_norm(x, sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], eps)
    h = gelu(h @ sd[pre + "mlp.fc1.weight"].t() + sd[pre + "mlp.fc1.bias"])
    return x + h @ sd[pre + "mlp.fc2.weight"].t() + sd[pre + "mlp.fc2.bias"]


def vit(img, sd, depth, heads, patch, eps=1e-6):
    """timm 0.4.x's VisionTransformer.forward in eval mode (the mean of both heads when distilled) in float64."""
    x = F.conv2d(img, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=patch).flatten(2).transpose(1, 2)
    tokens = [sd["cls_token"].expand(x.shape[0], -1, -1)]
    if "dist_token" in sd:
        tokens.append(sd["dist_token"].expand(x.shape[0], -1, -1))
    x = torch.cat(tokens + [x], dim=1) + sd["pos_embed"]
    for i in range(depth):
        x = block(x, sd, f"blocks.{i}.", heads, eps)
    x = plain_layer_norm(x, sd["norm.weight"], sd["norm.bias"], eps)
    out = x[:, 0] @ sd["head.weight"].t() + sd["head.bias"]
    if "dist_token" in sd:
        out = (out + x[:, 1] @ sd["head_dist.weight"].t() + sd["head_dist.bias"]) / 2
    return out


def tt_weight(cores, out_features, in_features):
    """The dense (out, in) weight a TT-matrix linear layer stands for (TTLinear.py:151-155): the cores (r_i, n_i, r_i+1)
    multiplied left to right, output modes first."""
    w = cores[0].reshape(-1, cores[0].shape[-1])
    for c in cores[1:]:
        w = w.reshape(-1, c.shape[0]) @ c.reshape(c.shape[0], -1)
    return w.reshape(out_features, in_features)


def state64(module, prefix="", requires_grad=False):
    """The module's state dict as float64 CPU leaves."""
    return {prefix + k: f64(v).requires_grad_(requires_grad) for k, v in module.state_dict().items()}


def with_tt_weights(sd, block_module, pre=""):
    """`sd` plus the dense weights of the block's TT-matrix projections, as differentiable functions of their cores."""
    sd = dict(sd)
    for name, lin in (("attn.qkv.", block_module.attn.qkv), ("attn.proj.", block_module.attn.proj),
                      ("mlp.fc1.", block_module.mlp.fc1), ("mlp.fc2.", block_module.mlp.fc2)):
        if pre + name + "weight" not in sd:
            cores = [sd[pre + name + f"tt_cores.{i}"] for i in range(len(lin.tt_cores))]
            sd[pre + name + "weight"] = tt_weight(cores, lin.out_features, lin.in_features)
    return sd
