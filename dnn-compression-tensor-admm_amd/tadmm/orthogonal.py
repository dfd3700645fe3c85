"""Orthogonality regulariser of the Tucker / SVD factors (the reference's orthogonal.py: append_double_l2_loss).

For every parameter whose name contains first_kernel, last_kernel, first_factor, last_factor or left_kernel, in
named_parameters() order, with P = squeeze(param):

    param.shape[0] < param.shape[1]:  E = P P^T - I      otherwise:  E = P^T P - I
    loss += 0.5 * rho * ||E||_F^2,    gradient 2 rho E P  (resp. 2 rho P E)

All matched factors of a model go through one native call (csrc/orth.hip): grouped fp64 Grams, one launch for every
E, gradient and partial norm, one fixed-order reduction.  The packed descriptors and the workspace are cached per
model, so a steady-state step uploads nothing.

Kept from the reference: substring selection, the orientation rule on the raw shape (square factors included), frozen
parameters that still add to the loss, and a RuntimeError for every factor torch.squeeze does not leave 2-D (rank 1,
a unit channel dimension, a k x k SVDConv2dC.left_kernel), raised before anything is launched.

Deliberate differences:
  * the reference adds into the caller's tensor (`loss += ...`); this returns `loss + term.to(loss.dtype)`, as
    ADMM.append_admm_loss does;
  * under torch.autocast the reference's torch.mm runs in fp16; here the value does not depend on autocast;
  * the Grams are accumulated in fp64 from the exact fp32 inputs, so the value keeps its digits near orthonormality,
    where the fp32 reference loses most of them;
  * parameters must be float32 HIP tensors on `device` ('cuda' without an index is the current device); anything
    else raises, naming the parameter.  There is no CPU fallback;
  * a raw shape with a unit size at index 0 or 1 that still squeezes to a matrix, such as (1, 4, 8) or (4, 1, 8),
    raises a RuntimeError.  The reference sizes its identity from the raw shape there and broadcasts eye(1), a value
    this does not reproduce.  The factorised layers never have such a shape.
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import List, Tuple

import torch

from ._cabi import Handle, OrthDesc, TadmmError

NAMES = ("first_kernel", "last_kernel", "first_factor", "last_factor", "left_kernel")


def select(model) -> List[Tuple[str, torch.nn.Parameter, bool]]:
    """The factors the reference regularises, in named_parameters() order: (name, param, gram_of_rows), where
    gram_of_rows means E = P P^T - I.  Host only; raises for a factor torch.squeeze does not leave 2-D."""
    out = []
    for name, p in model.named_parameters():
        if not any(k in name for k in NAMES):
            continue
        if p.dim() < 2:      # the reference's param.shape[1]
            raise IndexError(f"{name}: orthogonality regulariser needs at least 2 dimensions, got {tuple(p.shape)}")
        squeezed = [s for s in p.shape if s != 1]
        if len(squeezed) != 2:
            raise RuntimeError(f"{name}: torch.squeeze leaves shape {tuple(squeezed)} from {tuple(p.shape)}, "
                               "not a matrix")
        if p.shape[0] == 1 or p.shape[1] == 1:
            # e.g. (1, 4, 8): the reference sizes eye() from the raw shape and broadcasts eye(1) against the squeezed
            # Gram; no factorised layer has such a shape, so it is refused instead of computed differently
            raise RuntimeError(f"{name}: raw shape {tuple(p.shape)} has a unit dimension in front of the two that "
                               "torch.squeeze keeps; not supported")
        out.append((name, p, bool(p.shape[0] < p.shape[1])))
    return out


def _resolve(device) -> torch.device:
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


class _OrthPlan:
    """Packed descriptors + workspace of one set of factors (tadmm_orth_plan)."""

    def __init__(self, sel, dev: torch.device):
        self.device = dev
        self.h = Handle.get(dev.index)
        lib = self.h.lib
        n = len(sel)
        descs = (OrthDesc * n)()
        self.slots = []           # (offset, shape) of every gradient, in the order of the trainable factors
        goff = 0
        for i, (name, p, rows) in enumerate(sel):
            m = p.detach().squeeze()
            if m.stride(1) != 1 or m.stride(0) < m.shape[1]:
                raise TadmmError(-1, f"{name}: the factor must be stored row-major (strides {tuple(p.stride())})")
            d = descs[i]
            d.P = m.data_ptr()
            d.rows, d.cols, d.ld = int(m.shape[0]), int(m.shape[1]), int(m.stride(0))
            d.gram_of_rows = int(rows)
            if p.requires_grad:
                d.grad_offset = goff
                self.slots.append((goff, tuple(p.shape)))
                goff += (p.numel() + 15) // 16 * 16          # 64-byte aligned gradients
            else:
                d.grad_offset = -1
        self.gnumel = goff
        size = C.c_size_t()
        self.h.check(lib.tadmm_orth_workspace_bytes(n, descs, C.byref(size)))
        self.workspace = torch.empty(int(size.value), dtype=torch.uint8, device=dev)
        plan = C.c_void_p()
        self.h.check(lib.tadmm_orth_plan_create(self.h.ptr, n, descs, self.workspace.data_ptr(), int(size.value),
                                                torch.cuda.current_stream(dev).cuda_stream, C.byref(plan)))
        self._plan = plan
        self._fin = weakref.finalize(self, lib.tadmm_orth_plan_destroy, plan)

    def run(self, rho: float, want_grad: bool):
        dev = self.device
        loss = torch.zeros(1, dtype=torch.float64, device=dev)
        # fresh gradient storage per call: two losses alive in one step keep their own gradients
        flat = torch.empty(self.gnumel, dtype=torch.float32, device=dev) if (want_grad and self.gnumel) else None
        self.h.check(self.h.lib.tadmm_orth_l2(self._plan, float(rho), flat.data_ptr() if flat is not None else None,
                                              loss.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        grads = [] if flat is None else [flat[o:o + _numel(s)].view(s) for o, s in self.slots]
        return loss[0], grads


def _numel(shape) -> int:
    n = 1
    for s in shape:
        n *= s
    return n


_plans: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def _plan_for(model, sel, dev) -> _OrthPlan:
    key = (dev, tuple((name, p.data_ptr(), tuple(p.shape), p.requires_grad, rows) for name, p, rows in sel))
    ent = _plans.get(model)
    if ent is None or ent[0] != key:
        ent = (key, _OrthPlan(sel, dev))
        _plans[model] = ent
    return ent[1]


class _OrthFn(torch.autograd.Function):
    """loss + 0.5*rho*sum||E_i||^2; the forward computes the gradients, the backward scales them."""

    @staticmethod
    def forward(ctx, plan, rho, want_grad, loss, *params):
        val, grads = plan.run(rho, want_grad)
        ctx.grads = grads
        return loss + val.to(loss.dtype)

    @staticmethod
    def backward(ctx, gout):
        gs = torch._foreach_mul(ctx.grads, gout.to(torch.float32)) if ctx.grads else []
        return (None, None, None, gout) + tuple(gs)


def append_double_l2_loss(model, loss, rho, device):
    """orthogonal.py: append_double_l2_loss -- returns loss + 0.5*rho*sum_i ||E_i||_F^2 (see the module docstring)."""
    sel = select(model)
    if not sel:
        return loss
    dev = _resolve(device)
    for name, p, _ in sel:
        if not p.is_cuda or p.device != dev:
            raise TadmmError(-1, f"{name}: the factor lives on {p.device}, not on {dev}; there is no CPU path")
        if p.dtype != torch.float32:
            raise TadmmError(-1, f"{name}: the factor must be float32 (got {p.dtype})")
    plan = _plan_for(model, sel, dev)
    trainable = [p for _, p, _ in sel if p.requires_grad]
    want_grad = bool(trainable) and torch.is_grad_enabled()     # (forward itself runs with grad mode off)
    return _OrthFn.apply(plan, float(rho), want_grad, loss, *trainable)
