"""Float64 restatement of csrc/bnact.hip and of the ResNets of tadmm/resnet_cifar_layers.py and resnet_inet_layers.py.

timm is not installed where these tests run, so the reference's resnet_*_tt.py cannot be executed: this file is the
yardstick.  It is written from the formulas of the issue and from the forward methods of the reference's blocks:

    mean_c = mean over (n, h, w) of x,  var_c = mean of (x - mean_c)^2 (biased),  rstd_c = 1 / sqrt(var_c + eps)
    z = gamma_c (x - mean_c) rstd_c + beta_c + [c0 <= c < c0 + Cr] res[n, c - c0, h, w],   y = relu ? max(z, 0) : z
    running_mean <- (1 - momentum) running_mean + momentum mean_c
    running_var  <- (1 - momentum) running_var  + momentum var_c M / (M - 1),   M = N H W
    eval: a_c = gamma_c / sqrt(running_var_c + eps),  b_c = beta_c - running_mean_c a_c,  y = act(a x + b + res)

The tail's gradients are taken by float64 autograd over these formulas with the ReLU mask given from outside (the mask
of the route under test, from its own stored y), so the rounding of y is judged once, in the forward.  Factorised
convolutions enter as the dense weight their factors stand for, multiplied out in float64 (`dense_weight`); autograd
carries the gradients to the factors."""
import torch
import torch.nn.functional as F

F64 = torch.float64


def f64(t):
    return t.detach().to("cpu", F64)


def _window(res, c, c0):
    """The residual (N, Cr, H, W) as a (N, C, H, W) tensor that is zero outside the channels [c0, c0 + Cr)."""
    full = torch.zeros(res.shape[0], c, res.shape[2], res.shape[3], dtype=F64)
    return torch.cat([full[:, :c0], res, full[:, c0 + res.shape[1]:]], dim=1)


def batch_stats(x, eps=1e-5):
    X = f64(x)
    mean = X.mean(dim=(0, 2, 3))
    var = ((X - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
    return mean, var, 1.0 / torch.sqrt(var + eps)


def tail(x, gamma, beta, res=None, c0=0, relu=True, eps=1e-5):
    """dict of float64 tensors for the training-mode tail: y, z, mean, var, rstd and the elementwise error scale
    A = |gamma| (|x| + |mean|) rstd + |beta| + |res|."""
    X, gam, bet = f64(x), f64(gamma)[None, :, None, None], f64(beta)[None, :, None, None]
    mean, var, rstd = batch_stats(X, eps)
    m, r = mean[None, :, None, None], rstd[None, :, None, None]
    R = torch.zeros_like(X) if res is None else _window(f64(res), X.shape[1], c0)
    z = gam * (X - m) * r + bet + R
    return {"y": z.clamp_min(0) if relu else z, "z": z, "mean": mean, "var": var, "rstd": rstd,
            "A": gam.abs() * (X.abs() + m.abs()) * r + bet.abs() + R.abs()}


def tail_eval(x, running_mean, running_var, gamma, beta, res=None, c0=0, relu=True, eps=1e-5):
    """(y, error scale |a x| + |b| + |res|) of the folded eval formula."""
    X = f64(x)
    a = f64(gamma) / torch.sqrt(f64(running_var) + eps)
    b = f64(beta) - f64(running_mean) * a
    a, b = a[None, :, None, None], b[None, :, None, None]
    R = torch.zeros_like(X) if res is None else _window(f64(res), X.shape[1], c0)
    z = a * X + b + R
    return (z.clamp_min(0) if relu else z), (a * X).abs() + b.abs() + R.abs()


def running(running_mean, running_var, mean, var, M, momentum=0.1):
    return ((1 - momentum) * f64(running_mean) + momentum * mean,
            (1 - momentum) * f64(running_var) + momentum * var * M / (M - 1))


def tail_grads(x, gamma, beta, res, c0, g, mask=None, eps=1e-5):
    """dict dx, dres (None without res), dgamma, dbeta in float64 by autograd; `mask` (the shape of x, nonzero = the
    ReLU passes; None = no ReLU) comes from the stored output of the route being judged."""
    X, gam, bet = (f64(t).requires_grad_() for t in (x, gamma, beta))
    R = None if res is None else f64(res).requires_grad_()
    mean = X.mean(dim=(0, 2, 3), keepdim=True)
    var = ((X - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
    z = gam[None, :, None, None] * (X - mean) / torch.sqrt(var + eps) + bet[None, :, None, None]
    if R is not None:
        z = z + _window(R, X.shape[1], c0)
    if mask is not None:
        z = z * (f64(mask) != 0).to(F64)
    leaves = [X, gam, bet] + ([] if R is None else [R])
    grads = torch.autograd.grad(z, leaves, f64(g))
    return {"dx": grads[0], "dgamma": grads[1], "dbeta": grads[2], "dres": None if R is None else grads[3]}


# ---------------------------------------------------------------------------------------------------- the networks
def chain(cores):
    """core_0 (core_1 (...)) left to right (TTConv.py:313-319): the matrix (r_0 n_0 ... n_k-1, r_k)."""
    w = cores[0].reshape(-1, cores[0].shape[-1])
    for c in cores[1:]:
        w = w.reshape(-1, c.shape[0]) @ c.reshape(c.shape[0], -1)
    return w


def _cores(sd, pre, name):
    out, i = [], 0
    while f"{pre}{name}.{i}" in sd:
        out.append(sd[f"{pre}{name}.{i}"])
        i += 1
    return out


def dense_weight(sd, pre, conv):
    """The dense (O, I, kh, kw) kernel the convolution `conv` (a module; only its class and sizes are read) stands for,
    from the float64 state dict `sd` with keys pre + '<parameter>'."""
    kind = type(conv).__name__
    if pre + "weight" in sd:
        return sd[pre + "weight"]
    O, I = conv.out_channels, conv.in_channels
    kh, kw = conv.kernel_size
    if kind == "TTConv2dM":                     # per pixel: input cores (r, I), k x k core (r', r), output cores (O, r')
        w_in = chain(_cores(sd, pre, "in_tt_cores")).reshape(-1, I)
        w_out = chain(_cores(sd, pre, "out_tt_cores")).reshape(O, -1)
        return torch.einsum("os,srhw,ri->oihw", w_out, sd[pre + "core_kernel"], w_in)
    if kind == "TTConv2dR":                     # the flat (O, k^2, I) buffer read as (O, I, kh, kw), as TTConv.py:321-323
        w = chain(_cores(sd, pre, "out_tt_cores") + [sd[pre + "conv_core"]] + _cores(sd, pre, "in_tt_cores"))
        return w.reshape(O, kh * kw, I).reshape(O, I, kh, kw)
    if kind in ("TKConv2dC", "StfTKConv2dC"):
        return torch.einsum("os,srhw,ri->oihw", sd[pre + "last_kernel"][:, :, 0, 0], sd[pre + "core_kernel"],
                            sd[pre + "first_kernel"][:, :, 0, 0])
    if kind in ("TKConv2dM", "TKConv2dR"):
        core = sd[pre + ("core_kernel" if kind == "TKConv2dM" else "core_tensor")]
        return torch.einsum("os,srhw,ri->oihw", sd[pre + "last_factor"], core, sd[pre + "first_factor"])
    raise NotImplementedError(kind)


def conv(x, sd, pre, module):
    return F.conv2d(x, dense_weight(sd, pre, module), None, module.stride, module.padding)


def bn(x, sd, pre, training, res=None, c0=0, relu=True, eps=1e-5):
    """The tail in float64 under autograd, from the state dict's BatchNorm entries (not updated)."""
    gam, bet = sd[pre + "weight"][None, :, None, None], sd[pre + "bias"][None, :, None, None]
    if training:
        mean = x.mean(dim=(0, 2, 3), keepdim=True)
        var = ((x - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
    else:
        mean, var = sd[pre + "running_mean"][None, :, None, None], sd[pre + "running_var"][None, :, None, None]
    z = gam * (x - mean) / torch.sqrt(var + eps) + bet
    if res is not None:
        z = z + (res if res.shape[1] == x.shape[1] else _window(res, x.shape[1], c0))
    return z.clamp_min(0) if relu else z


def cifar_block(x, sd, pre, block, training):
    """resnet_cifar_tt.py: TTBasicBlock.forward; `block` gives the classes and the shortcut's kind."""
    out = bn(conv(x, sd, pre + "conv1.", block.conv1), sd, pre + "bn1.", training)
    out = conv(out, sd, pre + "conv2.", block.conv2)
    planes = out.shape[1]
    if pre + "shortcut.0.weight" in sd:                                                   # option B
        res = bn(F.conv2d(x, sd[pre + "shortcut.0.weight"], None, block.shortcut[0].stride), sd, pre + "shortcut.1.",
                 training, relu=False)
        return bn(out, sd, pre + "bn2.", training, res)
    if x.shape[1] != planes or x.shape[2] != out.shape[2]:                                # option A
        return bn(out, sd, pre + "bn2.", training, x[:, :, ::2, ::2], planes // 4)
    return bn(out, sd, pre + "bn2.", training, x)


def cifar_resnet(img, sd, model, training):
    out = bn(F.conv2d(img, sd["conv1.weight"], None, 1, 1), sd, "bn1.", training)
    for s, layer in enumerate((model.layer1, model.layer2, model.layer3), 1):
        for i, block in enumerate(layer):
            out = cifar_block(out, sd, f"layer{s}.{i}.", block, training)
    return out.mean(dim=(2, 3)) @ sd["linear.weight"].t() + sd["linear.bias"]


def inet_block(x, sd, pre, block, training):
    """resnet_inet_tt.py: TTBasicBlock.forward and TTBottleneck.forward."""
    names = [n for n in ("conv1", "conv2", "conv3") if hasattr(block, n)]
    identity = x
    if block.downsample is not None:
        identity = bn(F.conv2d(x, sd[pre + "downsample.0.weight"], None, block.downsample[0].stride), sd,
                      pre + "downsample.1.", training, relu=False)
    out = x
    for n in names[:-1]:
        out = bn(conv(out, sd, pre + n + ".", getattr(block, n)), sd, pre + "bn" + n[-1] + ".", training)
    n = names[-1]
    return bn(conv(out, sd, pre + n + ".", getattr(block, n)), sd, pre + "bn" + n[-1] + ".", training, identity)


def inet_resnet(img, sd, model, training):
    out = bn(F.conv2d(img, sd["conv1.weight"], None, 2, 3), sd, "bn1.", training)
    out = F.max_pool2d(out, 3, 2, 1)
    for s, layer in enumerate((model.layer1, model.layer2, model.layer3, model.layer4), 1):
        for i, block in enumerate(layer):
            out = inet_block(out, sd, f"layer{s}.{i}.", block, training)
    return out.mean(dim=(2, 3)) @ sd["fc.weight"].t() + sd["fc.bias"]


def state64(module, prefix="", requires_grad=False):
    """The module's state dict as float64 CPU leaves (the integer batch counters stay as they are)."""
    out = {}
    for k, v in module.state_dict().items():
        out[prefix + k] = f64(v).requires_grad_(requires_grad) if v.is_floating_point() else v.detach().cpu()
    return out
