"""Float64 restatement of csrc/dwbn.hip and of the MobileNetV2s of tadmm/mobilenet_cifar_layers.py and
mobilenet_inet_layers.py.

timm is not installed where these tests run, so the reference's mobilenetv2*_tt.py cannot be executed: this file is the
yardstick.  It is written from the formulas of the issue and from the forward methods of the reference's blocks:

    z[n,c,i,j] = sum_{a,b in 0..2} w[c,0,a,b] x[n,c, i s + a - 1, j s + b - 1]      (zero outside the plane; s = 1 or 2)
    mean_c, var_c (biased) over the M = N Ho Wo values of z,  rstd_c = 1 / sqrt(var_c + eps)
    y = min(max(gamma_c (z - mean_c) rstd_c + beta_c, 0), 6)
    eval: a_c = gamma_c / sqrt(running_var_c + eps),  b_c = beta_c - running_mean_c a_c,  y = clamp(a z + b)

The stage's gradients are written out (`stage_grads`), not taken from autograd: with gz = g [mask], xhat = (z - mean) rstd,

    dbeta = sum gz,  dgamma = sum gz xhat,  dz = gamma rstd (gz - dbeta / M - xhat dgamma / M),
    dx[n,c, i s + a - 1, j s + b - 1] += w[c,a,b] dz[n,c,i,j],   dw[c,a,b] = sum dz[n,c,i,j] x[n,c, i s + a - 1, j s + b - 1]

with the mask given from outside (that of the route under test, 0 < y < 6 of its own stored y), so the rounding of y is
judged once, in the forward.  tests/test_dwbn_host_cpu.py checks these formulas against autograd of F.conv2d."""
import torch
import torch.nn.functional as F

import _resnet_ref as R
from _resnet_ref import F64, f64, running, state64  # noqa: F401


def out_hw(h, w, s):
    return (h - 1) // s + 1, (w - 1) // s + 1


def _taps(Xp, ho, wo, s):
    """The nine shifted views of the padded input, (a, b) -> (N, C, Ho, Wo)."""
    return {(a, b): Xp[:, :, a:a + s * (ho - 1) + 1:s, b:b + s * (wo - 1) + 1:s] for a in range(3) for b in range(3)}


def dwconv(X, Wt, s):
    """The depthwise 3x3 convolution written out over its nine taps; X (N, C, H, W), Wt (C, 1, 3, 3), float64."""
    ho, wo = out_hw(X.shape[2], X.shape[3], s)
    Xp = F.pad(X, (1, 1, 1, 1))
    z = torch.zeros(X.shape[0], X.shape[1], ho, wo, dtype=X.dtype)
    for (a, b), v in _taps(Xp, ho, wo, s).items():
        z = z + Wt[None, :, 0, a, b, None, None] * v
    return z


def stage(x, w, gamma, beta, s, eps=1e-5):
    """dict of float64 tensors for the training-mode stage: y, z, mean, var, rstd and the elementwise error scale
    A = |gamma| (conv(|x|; |w|) + |mean|) rstd + |beta|."""
    X, Wt = f64(x), f64(w)
    gam, bet = f64(gamma)[None, :, None, None], f64(beta)[None, :, None, None]
    z = dwconv(X, Wt, s)
    mean = z.mean(dim=(0, 2, 3))
    var = ((z - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
    rstd = 1.0 / torch.sqrt(var + eps)
    m, r = mean[None, :, None, None], rstd[None, :, None, None]
    pre = gam * (z - m) * r + bet
    return {"y": pre.clamp(0, 6), "z": z, "mean": mean, "var": var, "rstd": rstd, "pre": pre,
            "A": gam.abs() * (dwconv(X.abs(), Wt.abs(), s) + m.abs()) * r + bet.abs()}


def stage_eval(x, w, running_mean, running_var, gamma, beta, s, eps=1e-5):
    """(y, error scale |a| conv(|x|; |w|) + |b|) of the folded eval formula."""
    X, Wt = f64(x), f64(w)
    a = f64(gamma) / torch.sqrt(f64(running_var) + eps)
    b = f64(beta) - f64(running_mean) * a
    a, b = a[None, :, None, None], b[None, :, None, None]
    return (a * dwconv(X, Wt, s) + b).clamp(0, 6), a.abs() * dwconv(X.abs(), Wt.abs(), s) + b.abs()


def stage_grads(x, w, gamma, beta, s, g, mask, eps=1e-5, st=None):
    """dict dx, dw, dgamma, dbeta in float64 from the formulas of the module docstring; `mask` (the shape of y, nonzero
    = the clamp passes) comes from the stored output of the route being judged.  `st` is `stage(...)` of the same
    inputs where the caller has it already."""
    X, Wt, gam = f64(x), f64(w), f64(gamma)[None, :, None, None]
    st = st or stage(x, w, gamma, beta, s, eps)
    z, m, r = st["z"], st["mean"][None, :, None, None], st["rstd"][None, :, None, None]
    M = z.shape[0] * z.shape[2] * z.shape[3]
    gz = f64(g) * (f64(mask) != 0).to(F64)
    xhat = (z - m) * r
    dbeta = gz.sum(dim=(0, 2, 3))
    dgamma = (gz * xhat).sum(dim=(0, 2, 3))
    dz = gam * r * (gz - dbeta[None, :, None, None] / M - xhat * dgamma[None, :, None, None] / M)
    ho, wo = z.shape[2], z.shape[3]
    Xp = F.pad(X, (1, 1, 1, 1))
    dXp = torch.zeros_like(Xp)
    dw = torch.zeros_like(Wt)
    for (a, b), v in _taps(Xp, ho, wo, s).items():
        dw[:, 0, a, b] = (dz * v).sum(dim=(0, 2, 3))
        dXp[:, :, a:a + s * (ho - 1) + 1:s, b:b + s * (wo - 1) + 1:s] += Wt[None, :, 0, a, b, None, None] * dz
    return {"dx": dXp[:, :, 1:-1, 1:-1], "dw": dw, "dgamma": dgamma, "dbeta": dbeta}


# ---------------------------------------------------------------------------------------------------- the networks
def pointwise(x, sd, pre):
    """A 1x1 convolution from the float64 state dict: dense (weight), SVDConv2dC (left_kernel (r, I, 1, 1), right_kernel
    (O, r, 1, 1)) or SVDConv2dM (left_factor (r, I), right_factor (O, r)), the factors multiplied out in float64."""
    if pre + "weight" in sd:
        return F.conv2d(x, sd[pre + "weight"])
    if pre + "left_kernel" in sd:
        return F.conv2d(F.conv2d(x, sd[pre + "left_kernel"]), sd[pre + "right_kernel"])
    if pre + "left_factor" in sd:
        w = sd[pre + "right_factor"] @ sd[pre + "left_factor"]
        return F.conv2d(x, w[:, :, None, None])
    raise NotImplementedError(pre)


def relu6(x):
    return x.clamp(0, 6)


def depthwise(x, sd, pre, s):
    return dwconv(x, sd[pre + "weight"], s)


def cifar_block(x, sd, pre, block, training):
    """mobilenetv2_cifar_tt.py: TTBaseBlock.forward; `block` gives the stride and whether there is a shortcut."""
    out = relu6(R.bn(pointwise(x, sd, pre + "conv1."), sd, pre + "bn1.", training, relu=False))
    out = relu6(R.bn(depthwise(out, sd, pre + "conv2.", block.stride), sd, pre + "bn2.", training, relu=False))
    return R.bn(pointwise(out, sd, pre + "conv3."), sd, pre + "bn3.", training, x if block.shortcut else None, relu=False)


def cifar_mobilenet(img, sd, model, training):
    out = relu6(R.bn(F.conv2d(img, sd["conv0.weight"], None, 1, 1), sd, "bn0.", training, relu=False))
    for i, block in enumerate(model.bottlenecks):
        out = cifar_block(out, sd, f"bottlenecks.{i}.", block, training)
    out = relu6(R.bn(pointwise(out, sd, "conv1."), sd, "bn1.", training, relu=False))
    return out.mean(dim=(2, 3)) @ sd["fc.weight"].t() + sd["fc.bias"]


def inet_block(x, sd, pre, block, training):
    """mobilenetv2_tt.py: TTInvertedResidual.forward with its two Sequential layouts."""
    out, k = x, 0
    if block.expanded:
        out, k = relu6(R.bn(pointwise(x, sd, pre + "conv.0."), sd, pre + "conv.1.", training, relu=False)), 3
    s = block.conv[k].stride[0]
    out = relu6(R.bn(depthwise(out, sd, f"{pre}conv.{k}.", s), sd, f"{pre}conv.{k + 1}.", training, relu=False))
    return R.bn(pointwise(out, sd, f"{pre}conv.{k + 3}."), sd, f"{pre}conv.{k + 4}.", training,
                x if block.identity else None, relu=False)


def inet_mobilenet(img, sd, model, training):
    out = relu6(R.bn(F.conv2d(img, sd["features.0.0.weight"], None, 2, 1), sd, "features.0.1.", training, relu=False))
    for i in range(1, len(model.features)):
        out = inet_block(out, sd, f"features.{i}.", model.features[i], training)
    out = relu6(R.bn(pointwise(out, sd, "conv.0."), sd, "conv.1.", training, relu=False))
    return out.mean(dim=(2, 3)) @ sd["classifier.weight"].t() + sd["classifier.bias"]
