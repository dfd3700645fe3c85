"""Generate golden vectors G15 (the distillation criterion) from the REAL reference.

    python tests/golden/make_golden_distill.py <path of the reference checkout>

Runs only where the reference is at hand.  Loads its losses.py as a module object and calls the reference's OWN
`DistillationLoss` on the CPU in float32, around torch.nn.CrossEntropyLoss (plain, with label smoothing, and with
probability targets), with a teacher module that returns fixed logits.  Recorded per case: the logits, the teacher's
logits, the targets, the loss and the autograd gradients of both logit tensors.  The case list goes to
g15_distill.json.  The reference never travels with the tests; these data files do.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

SHAPES = [(2, 3), (5, 10), (7, 100), (3, 257)]
# (distillation type, tau, alpha, criterion, outputs as a tuple)
VARIANTS = [("none", 1.0, 0.5, "ce", False), ("soft", 1.0, 0.5, "ce", True), ("soft", 3.0, 0.5, "ce_ls", False),
            ("hard", 1.0, 0.5, "ce_prob", True), ("hard", 1.0, 0.5, "ce_ls", False), ("soft", 3.0, 0.5, "ce_prob", True)]
EXTRA = [((5, 10), ("soft", 3.0, 0.0, "ce", True)), ((7, 100), ("hard", 1.0, 1.0, "ce", True)),
         ((5, 10), ("none", 1.0, 0.5, "ce_prob", True))]


class FixedTeacher(torch.nn.Module):
    def __init__(self, logits):
        super().__init__()
        self.logits = logits

    def forward(self, x):
        return self.logits


def load(path):
    spec = importlib.util.spec_from_file_location("ref_losses", os.path.join(path, "losses.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(path):
    mod = load(path)
    rec, index = {}, []
    todo = [(shape, v) for shape in SHAPES for v in VARIANTS] + EXTRA
    for n, ((B, C), (kind, tau, alpha, crit, tup)) in enumerate(todo):
        name = f"c{n:02d}"
        g = torch.Generator().manual_seed(1500 + n)
        s = (2.0 * torch.randn(B, C, generator=g)).requires_grad_(True)
        k = (2.0 * torch.randn(B, C, generator=g)).requires_grad_(True) if tup else None
        t = 2.0 * torch.randn(B, C, generator=g)
        if crit == "ce_prob":
            target = torch.softmax(1.5 * torch.randn(B, C, generator=g), dim=1)
        else:
            target = torch.randint(0, C, (B,), generator=g)
        criterion = torch.nn.CrossEntropyLoss(label_smoothing=0.1) if crit == "ce_ls" else torch.nn.CrossEntropyLoss()
        loss_fn = mod.DistillationLoss(criterion, FixedTeacher(t), kind, alpha, tau)
        loss = loss_fn(torch.zeros(B, 1), (s, k) if tup else s, target)
        loss.backward()
        rec[f"{name}.s"], rec[f"{name}.t"], rec[f"{name}.target"] = s.detach().numpy(), t.numpy(), target.numpy()
        rec[f"{name}.loss"] = loss.detach().numpy().reshape(1)
        rec[f"{name}.grad_s"] = (s.grad if s.grad is not None else torch.zeros_like(s)).numpy()
        if tup:
            rec[f"{name}.k"] = k.detach().numpy()
            rec[f"{name}.grad_k"] = (k.grad if k.grad is not None else torch.zeros_like(k)).numpy()
        index.append(dict(name=name, B=B, C=C, type=kind, tau=tau, alpha=alpha, criterion=crit, tuple=tup))
    dst = os.path.join(HERE, "g15_distill.npz")
    np.savez_compressed(dst, **rec)
    with open(os.path.join(HERE, "g15_distill.json"), "w") as f:
        json.dump({"cases": index}, f, indent=1)
    print(dst, os.path.getsize(dst), "bytes,", len(index), "cases")


if __name__ == "__main__":
    main(sys.argv[1])
