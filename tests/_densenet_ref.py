"""Float64 restatement of csrc/densebn.hip and of the DenseNets of tadmm/densenet_cifar_layers.py and
densenet_inet_layers.py.

timm is not installed where these tests run, so the reference's densenet_*_tt.py cannot be executed: this file is the
yardstick.  It is written in plain torch with an explicit `torch.cat`, from the formulas of the issue and from the forward
methods of the reference's blocks:

    X = cat(features, 1);  mean_c = mean over (n, h, w) of X,  var_c = mean of (X - mean_c)^2 (biased)
    y = act(gamma_c (X - mean_c) / sqrt(var_c + eps) + beta_c)
    running_mean <- (1 - momentum) running_mean + momentum mean_c
    running_var  <- (1 - momentum) running_var  + momentum var_c M / (M - 1),   M = N H W
    eval: a_c = gamma_c / sqrt(running_var_c + eps),  b_c = beta_c - running_mean_c a_c,  y = act(a X + b)

Gradients are taken by float64 autograd over these formulas with the ReLU mask given from outside (the mask of the route
under test, from its own stored y), so the rounding of y is judged once, in the forward.  Factorised convolutions enter
as the dense weight their factors stand for, multiplied out in float64 (`_resnet_ref.dense_weight`)."""
import torch
import torch.nn.functional as F

import _resnet_ref as R
from _resnet_ref import F64, f64, state64  # noqa: F401


def pre_act(segments, gamma, beta, relu=True, eps=1e-5):
    """dict of float64 tensors for the training-mode pre-activation of a list of feature tensors: y, mean, var."""
    X = torch.cat([f64(s) for s in segments], 1)
    mean, var, rstd = R.batch_stats(X, eps)
    z = f64(gamma)[None, :, None, None] * (X - mean[None, :, None, None]) * rstd[None, :, None, None] \
        + f64(beta)[None, :, None, None]
    return {"y": z.clamp_min(0) if relu else z, "mean": mean, "var": var}


def pre_act_eval(segments, running_mean, running_var, gamma, beta, relu=True, eps=1e-5):
    X = torch.cat([f64(s) for s in segments], 1)
    a = f64(gamma) / torch.sqrt(f64(running_var) + eps)
    b = f64(beta) - f64(running_mean) * a
    z = a[None, :, None, None] * X + b[None, :, None, None]
    return z.clamp_min(0) if relu else z


def pre_act_graph(leaves, gamma, beta, mask=None, eps=1e-5):
    """The pre-activation under float64 autograd; `leaves`, `gamma`, `beta` are float64 tensors of a graph, `mask` (the
    shape of y, nonzero = the ReLU passes; None = no ReLU) comes from the stored output of the route being judged."""
    X = torch.cat(list(leaves), 1)
    mean = X.mean(dim=(0, 2, 3), keepdim=True)
    var = ((X - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
    z = gamma[None, :, None, None] * (X - mean) / torch.sqrt(var + eps) + beta[None, :, None, None]
    return z if mask is None else z * (f64(mask) != 0).to(F64)


def pre_act_grads(segments, gamma, beta, g, mask=None, eps=1e-5):
    """dict dx (a list, one per segment), dgamma, dbeta in float64 by autograd."""
    leaves = [f64(s).requires_grad_() for s in segments]
    gam, bet = f64(gamma).requires_grad_(), f64(beta).requires_grad_()
    z = pre_act_graph(leaves, gam, bet, mask, eps)
    grads = torch.autograd.grad(z, leaves + [gam, bet], f64(g))
    return {"dx": list(grads[:len(leaves)]), "dgamma": grads[-2], "dbeta": grads[-1]}


# ---------------------------------------------------------------------------------------------------- the networks
def cifar_layer(x, sd, pre, layer, training):
    """densenet_cifar_tt.py: TenBasicBlock.forward / TenBottleneckBlock.forward without dropout: cat([x, out], 1)."""
    out = R.conv(R.bn(x, sd, pre + "bn1.", training), sd, pre + "conv1.", layer.conv1)
    if hasattr(layer, "conv2"):
        out = R.conv(R.bn(out, sd, pre + "bn2.", training), sd, pre + "conv2.", layer.conv2)
    return torch.cat([x, out], 1)


def cifar_dense_block(x, sd, pre, block, training):
    for i, layer in enumerate(block.layer):
        x = cifar_layer(x, sd, f"{pre}layer.{i}.", layer, training)
    return x


def cifar_transition(x, sd, pre, trans, training):
    return F.avg_pool2d(R.conv(R.bn(x, sd, pre + "bn1.", training), sd, pre + "conv1.", trans.conv1), 2)


def cifar_densenet(img, sd, model, training):
    out = F.conv2d(img, sd["conv1.weight"], None, 1, 1)
    out = cifar_transition(cifar_dense_block(out, sd, "block1.", model.block1, training), sd, "trans1.", model.trans1, training)
    out = cifar_transition(cifar_dense_block(out, sd, "block2.", model.block2, training), sd, "trans2.", model.trans2, training)
    out = cifar_dense_block(out, sd, "block3.", model.block3, training)
    out = R.bn(out, sd, "bn1.", training)
    out = F.avg_pool2d(out, 8).reshape(-1, model.in_planes)
    return out @ sd["fc.weight"].t() + sd["fc.bias"]


def inet_dense_block(x, sd, pre, block, training):
    """densenet_inet_tt.py: TenDenseBlock.forward with TenDenseLayer.forward, norm = BatchNorm + ReLU, no dropout."""
    features = [x]
    for name, layer in block.items():
        p = f"{pre}{name}."
        out = R.conv(R.bn(torch.cat(features, 1), sd, p + "norm1.", training), sd, p + "conv1.", layer.conv1)
        features.append(R.conv(R.bn(out, sd, p + "norm2.", training), sd, p + "conv2.", layer.conv2))
    return torch.cat(features, 1)


def inet_transition(x, sd, pre, trans, training):
    return F.avg_pool2d(R.conv(R.bn(x, sd, pre + "norm.", training), sd, pre + "conv.", trans.conv), 2, 2)


def inet_densenet(img, sd, model, training):
    """The plain stem (conv0 7x7 / 2, norm0, 3x3 / 2 max pool), the blocks and transitions, norm5, average pool, classifier."""
    f = model.features
    out = R.bn(F.conv2d(img, sd["features.conv0.weight"], None, 2, 3), sd, "features.norm0.", training)
    out = F.max_pool2d(out, 3, 2, 1)
    s = 1
    while hasattr(f, f"denseblock{s}"):
        out = inet_dense_block(out, sd, f"features.denseblock{s}.", getattr(f, f"denseblock{s}"), training)
        if hasattr(f, f"transition{s}"):
            out = inet_transition(out, sd, f"features.transition{s}.", getattr(f, f"transition{s}"), training)
        s += 1
    out = R.bn(out, sd, "features.norm5.", training)
    return out.mean(dim=(2, 3)) @ sd["classifier.weight"].t() + sd["classifier.bias"]
