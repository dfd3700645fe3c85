"""Generate golden vectors G20 (TinyBERT's intermediate-layer losses) from the REAL reference.

    python tests/golden/make_golden_layer_mse.py <path of the reference checkout>

Runs only where the reference is at hand.  Reads xcompression/task_distill.py, takes the lines of its training loop from
the one containing `new_teacher_atts = teacher_atts[-1]` through the one containing `loss = rep_loss + att_loss`,
dedents them and executes them -- the reference's OWN statements, on the CPU in float32 -- in a namespace that holds
`torch`, `device`, `loss_mse = MSELoss()`, the two running sums and the four lists of per-layer tensors.  Recorded per
case: the last layer's student and teacher attention scores and hidden states, the two losses and the autograd gradients
of the two student tensors.  The case list goes to g20_layer_mse.json.  The reference's text is never written anywhere;
these data files travel with the tests.

Scores are randn + mask with a (B, 1, 1, S) additive mask of -10000 over a per-sample suffix of the keys, as the BERT
models of the reference build it; in the "differ" cases student and teacher are given different suffixes.
"""
import json
import os
import sys
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

SHAPES = [(1, 1, 1, 1), (2, 2, 5, 4), (3, 2, 9, 7), (2, 3, 37, 5)]      # (B, H, S, D)
FIRST, LAST = "new_teacher_atts = teacher_atts[-1]", "loss = rep_loss + att_loss"


def block(path):
    lines = open(os.path.join(path, "xcompression", "task_distill.py")).read().splitlines()
    a = next(i for i, ln in enumerate(lines) if FIRST in ln)
    b = next(i for i, ln in enumerate(lines) if i >= a and LAST in ln)
    return compile(textwrap.dedent("\n".join(lines[a:b + 1])), "task_distill_block", "exec")


def suffix_mask(B, S, lengths):
    """(B, 1, 1, S): 0 over the first lengths[b] keys of sample b, -10000 over the rest."""
    m = torch.zeros(B, 1, 1, S)
    for b, n in enumerate(lengths):
        m[b, 0, 0, n:] = -10000.0
    return m


def kept_lengths(B, S, shift):
    """Kept keys per sample: between 15 % and 50 % of the S keys are masked, the count moved on by `shift` for the
    other side; a single key is kept, or masked under `shift`."""
    if S == 1:
        return [1 - shift] * B
    lo = -(-15 * S // 100)
    span = max(2, S // 2 - lo)
    return [S - (lo + (b + shift) % span) for b in range(B)]


def main(path):
    code = block(path)
    rec, index = {}, []
    n = 0
    for (B, H, S, D) in SHAPES:
        for differ in (False, True):
            name = f"c{n:02d}"
            g = torch.Generator().manual_seed(2000 + n)
            lt = kept_lengths(B, S, 0)
            ls = lt if not differ else (kept_lengths(B, S, 1) if B == 1 else lt[-1:] + lt[:-1])   # both ways when B > 1
            s_att = (torch.randn(B, H, S, S, generator=g) + suffix_mask(B, S, ls)).requires_grad_(True)
            t_att = torch.randn(B, H, S, S, generator=g) + suffix_mask(B, S, lt)
            s_rep = torch.randn(B, S, D, generator=g).requires_grad_(True)
            t_rep = torch.randn(B, S, D, generator=g)
            ns = dict(torch=torch, device="cpu", loss_mse=torch.nn.MSELoss(), att_loss=0., rep_loss=0.,
                      student_atts=[s_att], teacher_atts=[t_att], student_reps=[s_rep], teacher_reps=[t_rep])
            exec(code, ns)
            ns["loss"].backward()
            rec[f"{name}.s_att"], rec[f"{name}.t_att"] = s_att.detach().numpy(), t_att.numpy()
            rec[f"{name}.s_rep"], rec[f"{name}.t_rep"] = s_rep.detach().numpy(), t_rep.numpy()
            rec[f"{name}.att_loss"] = ns["att_loss"].detach().numpy().reshape(1)
            rec[f"{name}.rep_loss"] = ns["rep_loss"].detach().numpy().reshape(1)
            rec[f"{name}.grad_att"], rec[f"{name}.grad_rep"] = s_att.grad.numpy(), s_rep.grad.numpy()
            index.append(dict(name=name, B=B, H=H, S=S, D=D, differ=differ, kept_student=ls, kept_teacher=lt))
            n += 1
    dst = os.path.join(HERE, "g20_layer_mse.npz")
    np.savez_compressed(dst, **rec)
    with open(os.path.join(HERE, "g20_layer_mse.json"), "w") as f:
        json.dump({"cases": index}, f, indent=1)
    print(dst, os.path.getsize(dst), "bytes,", len(index), "cases")


if __name__ == "__main__":
    main(sys.argv[1])
