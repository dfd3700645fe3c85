"""Generate golden vectors G8 (the SVD layers of SVDConv.py) from the REAL reference.

Runs ONLY in the build container: imports the reference's SVDConv.py (numpy + torch only) and records inputs, outputs,
state_dicts, `forward_flops` and the constructor errors as small .npz / .json fixtures.  The reference never travels
to the GPU box; these data files do.

Weights have a clear spectral gap after rank r and distinct leading singular values, so the rank-r truncation and its
singular vectors (up to sign) are unique at fp32 precision.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

import SVDConv as ref  # noqa: E402


class HP:
    def __init__(self, ranks):
        self.ranks = ranks


def gapped(o, i, r, rng):
    """(O, I, 1, 1) float32 weight: leading singular values 2 * 0.85^j (j < r), the rest below 1e-4."""
    k = min(o, i)
    q1, _ = np.linalg.qr(rng.standard_normal((o, k)))
    q2, _ = np.linalg.qr(rng.standard_normal((i, k)))
    s = np.concatenate([2.0 * 0.85 ** np.arange(r), 1e-4 * rng.uniform(0.1, 1.0, k - r)])
    return ((q1 * s) @ q2.T).astype(np.float32)[:, :, None, None]


# name: (class, in, out, rank, bias, padding, x shape (B, H, W))
CASES = {
    "mbv2c_C_bias": ("C", 24, 144, 18, True, 0, (2, 6, 6)),       # bottlenecks.3.conv1 of svd_mobilenetv2_cifar
    "mbv2c_C_nobias": ("C", 24, 144, 18, False, 0, (2, 6, 6)),
    "mbv2c_M_bias": ("M", 24, 144, 18, True, 0, (2, 6, 6)),
    "mbv2c_M_nobias": ("M", 24, 144, 18, False, 0, (2, 6, 6)),
    "r50_C_7x7": ("C", 64, 256, 32, True, 0, (2, 7, 7)),         # layer1.x.conv3 of tk_resnet50 3x, 7x7 plane
    "C_pad1": ("C", 16, 32, 8, True, 1, (2, 5, 5)),
    "R_dense": ("R", 32, 48, 12, True, 0, (2, 6, 6)),
}

# constructor error cases: (class, kwargs)
ERRORS = {
    "R_kernel_tuple": ("R", dict(kernel_size=(1, 1))),
    "R_kernel3": ("R", dict(kernel_size=3)),
    "R_stride2": ("R", dict(kernel_size=1, stride=2)),
    "R_reset_in_ne_out": ("R", dict(kernel_size=1, in_channels=16, out_channels=24)),
    "C_padding_mode": ("C", dict(padding_mode="reflect")),
    "C_groups": ("C", dict(groups=2)),
    "C_kernel3": ("C", dict(kernel_size=3)),
    "C_stride2": ("C", dict(stride=2)),
    "M_padding_mode": ("M", dict(padding_mode="circular")),
    "M_groups": ("M", dict(groups=4)),
    "M_kernel3": ("M", dict(kernel_size=(3, 3))),
    "M_stride2": ("M", dict(stride=(1, 2))),
}

# parameter names / shapes without dense_w: (class, in, out, rank, bias)
PLAIN = {
    "R_plain": ("R", 16, 16, 4, True),
    "R_plain_nobias": ("R", 16, 16, 4, False),
    "C_plain": ("C", 24, 40, 6, True),
    "C_plain_nobias": ("C", 24, 40, 6, False),
    "M_plain": ("M", 24, 40, 6, True),
    "M_plain_nobias": ("M", 24, 40, 6, False),
}

CLASSES = {"R": ref.SVDConv2dR, "C": ref.SVDConv2dC, "M": ref.SVDConv2dM}


def main():
    rng = np.random.default_rng(20220206)
    torch.manual_seed(0)
    out, meta = {}, {"cases": {}, "errors": {}, "plain": {}}
    for key, (cls, cin, cout, r, bias, pad, (b, h, w)) in CASES.items():
        wd = gapped(cout, cin, r, rng)
        bd = rng.standard_normal(cout).astype(np.float32) if bias else None
        x = rng.standard_normal((b, cin, h, w)).astype(np.float32)
        layer = CLASSES[cls](cin, cout, 1, padding=pad, bias=bias, hp_dict=HP({"l.weight": r}), name="l.weight",
                             dense_w=torch.from_numpy(wd), dense_b=None if bd is None else torch.from_numpy(bd))
        with torch.no_grad():
            y = layer(torch.from_numpy(x)).contiguous().numpy()
        out[key + "_w"], out[key + "_x"], out[key + "_y"] = wd, x, y
        if bd is not None:
            out[key + "_b"] = bd
        names = []
        for n, t in layer.state_dict().items():
            names.append([n, list(t.shape)])
            out[f"{key}_sd_{n}"] = t.detach().numpy()
        m = dict(cls=cls, in_channels=cin, out_channels=cout, rank=r, bias=bias, padding=pad, state_dict=names)
        if cls == "C":
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf), torch.no_grad():
                _, base_flops, compr_flops = layer.forward_flops(torch.from_numpy(x))
            m.update(base_flops=base_flops, compr_flops=compr_flops, flops_line=buf.getvalue(),
                     extra_repr=layer.extra_repr())
        meta["cases"][key] = m
    for key, (cls, kw) in ERRORS.items():
        args = dict(in_channels=16, out_channels=16, kernel_size=1, hp_dict=HP({"l.weight": 4}), name="l.weight")
        args.update(kw)
        try:
            CLASSES[cls](**args)
            raise AssertionError(f"{key}: the reference did not raise")
        except AssertionError:
            raise
        except Exception as e:  # noqa: BLE001 -- the exception type is what is recorded
            meta["errors"][key] = dict(cls=cls, kwargs=kw, type=type(e).__name__, message=str(e))
    for key, (cls, cin, cout, r, bias) in PLAIN.items():
        layer = CLASSES[cls](cin, cout, 1, bias=bias, hp_dict=HP({"l.weight": r}), name="l.weight")
        meta["plain"][key] = dict(cls=cls, in_channels=cin, out_channels=cout, rank=r, bias=bias,
                                  state_dict=[[n, list(t.shape)] for n, t in layer.state_dict().items()])
    np.savez_compressed(os.path.join(HERE, "g8_svd_layers.npz"), **out)
    json.dump(meta, open(os.path.join(HERE, "g8_svd_layers.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
