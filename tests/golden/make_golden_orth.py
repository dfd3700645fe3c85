"""Generate golden vectors G9 (the orthogonality regulariser of orthogonal.py) from the REAL reference.

Runs ONLY in the build container: imports the reference's orthogonal.py (torch only) and records, for small modules
whose parameters carry the reference's names, the loss and every gradient of `append_double_l2_loss` in fp32, the same
call on fp64 copies of the parameters (torch.eye promotes, so this is an fp64 result of the reference's own code),
which parameters it regularised and the errors it raises.  Only these data files travel to the GPU box.
"""
import copy
import json
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

import orthogonal as ref  # noqa: E402

RHO = 0.1

# case: list of (dotted name, shape, requires_grad); modules are created along the dotted path in this order
CASES = {
    # TKConv2dC-like: 4-D (r, C, 1, 1) kernels, wide / tall / square, a non-matching core and bias
    "tk_conv": [("layer1.0.conv1.first_kernel", (6, 16, 1, 1), True), ("layer1.0.conv1.core_kernel", (8, 6, 3, 3), True),
                ("layer1.0.conv1.last_kernel", (24, 8, 1, 1), True), ("layer1.0.conv1.bias", (24,), True),
                ("layer2.conv.first_kernel", (5, 5, 1, 1), True), ("layer2.conv.last_kernel", (7, 7, 1, 1), True)],
    # TKLinearM-like: 2-D factors, wide / tall / square
    "tk_linear": [("fc.first_factor", (6, 40), True), ("fc.core_tensor", (8, 6), True), ("fc.last_factor", (48, 8), True),
                  ("fc.bias", (48,), True), ("head.first_factor", (9, 9), True), ("head.last_factor", (12, 12), True)],
    # SVD layers: left_kernel matches, left_factor / right_* do not
    "svd": [("conv.left_factor", (10, 4), True), ("conv.right_factor", (4, 10), True),
            ("conv2.left_kernel", (4, 12, 1, 1), True), ("conv2.right_kernel", (16, 4, 1, 1), True)],
    # a frozen factor still adds to the loss
    "frozen": [("blk.first_factor", (5, 20), False), ("blk.last_factor", (20, 5), True),
               ("blk.sub.first_kernel", (3, 9, 1, 1), True)],
    # the smallest Tucker factors of tk_resnet32 (n = 8, K = 16)
    "small": [("layer1.0.conv1.first_kernel", (8, 16, 1, 1), True), ("layer1.0.conv1.last_kernel", (16, 8, 1, 1), True)],
    # several 32-row tiles and a split reduction
    "multi_tile": [("features.first_kernel", (40, 160, 1, 1), True), ("features.last_kernel", (300, 40, 1, 1), True),
                   ("classifier.last_factor", (33, 33), True)],
    # nothing to regularise
    "no_match": [("conv.weight", (8, 4, 3, 3), True), ("fc.weight", (10, 8), True), ("fc.core_tensor", (4, 4), True)],
}

# the reference raises on these (torch.squeeze does not leave a matrix); a valid factor comes first
ERRORS = {
    "rank1": [("a.first_factor", (4, 9), True), ("b.first_kernel", (1, 8, 1, 1), True)],
    "unit_channel": [("a.first_factor", (4, 9), True), ("b.last_kernel", (6, 1, 1, 1), True)],
    "left_kernel_3x3": [("a.first_factor", (4, 9), True), ("conv.left_kernel", (3, 8, 3, 3), True)],
}


def draw(rng, shape):
    """float32 values of scale 1/sqrt(long side) (at most 0.3): E = O(1), where the fp32 reference keeps its digits"""
    long_side = max(int(np.prod(shape[1:])) if len(shape) > 1 else 1, shape[0])
    return (rng.standard_normal(shape) * min(0.3, long_side ** -0.5)).astype(np.float32)


def build(spec, values):
    root = torch.nn.Module()
    for name, shape, rg in spec:
        *path, leaf = name.split(".")
        m = root
        for part in path:
            if not hasattr(m, part):
                m.add_module(part, torch.nn.Module())
            m = getattr(m, part)
        m.register_parameter(leaf, torch.nn.Parameter(torch.from_numpy(values[name]).clone(), requires_grad=rg))
    return root


def run(model, dtype):
    loss = torch.zeros((), dtype=dtype)
    out = ref.append_double_l2_loss(model, loss, RHO, "cpu")
    if out.requires_grad:
        out.backward()
    return out, {n: (None if p.grad is None else p.grad.detach().numpy()) for n, p in model.named_parameters()}


def main():
    rng = np.random.default_rng(20211115)
    torch.manual_seed(0)
    out, meta = {}, {"rho": RHO, "cases": {}, "errors": {}}
    for key, spec in CASES.items():
        values = {n: draw(rng, s) for n, s, _ in spec}
        model = build(spec, values)
        order = [n for n, _ in model.named_parameters()]
        l32, g32 = run(model, torch.float32)
        m64 = build(spec, {n: v.astype(np.float64) for n, v in values.items()})
        l64, g64 = run(m64, torch.float64)
        # matched = the parameters the reference differentiates when every parameter is trainable
        probe = copy.deepcopy(m64)
        for p in probe.parameters():
            p.requires_grad_(True)
        _, gp = run(probe, torch.float64)
        matched = [n for n in order if gp[n] is not None]
        shapes = dict((n, s) for n, s, _ in spec)
        for n in order:
            out[f"{key}__{n}"] = values[n]
            if g32[n] is not None:
                out[f"{key}__grad32__{n}"] = g32[n]
                out[f"{key}__grad64__{n}"] = g64[n]
        meta["cases"][key] = dict(
            params=[[n, list(s), rg] for n, s, rg in spec], order=order, matched=matched,
            gram_of_rows={n: bool(shapes[n][0] < shapes[n][1]) for n in matched},
            loss32=float(l32.detach()), loss64=float(l64.detach()), with_grad=[n for n in order if g32[n] is not None])
    for key, spec in ERRORS.items():
        values = {n: draw(rng, s) for n, s, _ in spec}
        model = build(spec, values)
        try:
            run(model, torch.float32)
            raise AssertionError(f"{key}: the reference did not raise")
        except AssertionError:
            raise
        except Exception as e:  # noqa: BLE001 -- the exception type is what is recorded
            meta["errors"][key] = dict(params=[[n, list(s), rg] for n, s, rg in spec], type=type(e).__name__,
                                       message=str(e), failing=spec[-1][0])
    np.savez_compressed(os.path.join(HERE, "g9_orthogonal.npz"), **out)
    json.dump(meta, open(os.path.join(HERE, "g9_orthogonal.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
