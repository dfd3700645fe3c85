"""Riemannian SGD for models with Stiefel factors (`StfTKConv2dC`): what the reference gets from
`geoopt.optim.RiemannianSGD` for every model whose name starts with `stf` (engines.py:167-174).

`StiefelSGD(params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False)` is a `torch.optim.Optimizer`:

  * parameters with `manifold == "stiefel"` (`StiefelParameter`) and a gradient go through ONE native launch per param
    group (csrc/stiefel.hip, `ops.StiefelPlan`).  With sym(A) = (A + A^T) / 2:
        g = grad + weight_decay X;   r = g - X sym(X^T g)              tangent projection, embedded metric
        M <- momentum M + (1 - dampening) r;   d = nesterov ? r + momentum M : M        (d = r without momentum)
        X <- qr(X - lr d).Q with diag(R) > 0;   M <- M - X sym(X^T M)   QR retraction, transport by projection
    The plan of a group owns a flat gradient buffer; a step stages the gradients into it with one `_foreach_copy_` and
    leaves `.grad` pointing at the views, so gradients that are zeroed in place (`zero_grad(set_to_none=False)`)
    accumulate there directly and nothing is staged.  The plan is rebuilt when the set of factors with a gradient, a
    factor's storage or a momentum buffer changes (that costs one table upload);
  * all other parameters take torch's ordinary SGD update with the same hyper-parameters (an inner `torch.optim.SGD`
    sharing this optimiser's state);
  * `step()` never synchronises.  A factor whose retraction broke down (a rank-deficient X - lr d, a non-finite
    gradient) keeps X and M; `failed()` names those factors at the cost of one synchronisation;
  * `state_dict` / `load_state_dict` round-trip the momentum buffers (`state[p]["momentum_buffer"]`, as torch's SGD).

Differences from geoopt, both deliberate:
  * the momentum buffer starts at ZERO, so the first step moves along (1 - dampening) r.  geoopt seeds the buffer
    differently on its first step (from memory of its source: with the gradient itself, like torch's SGD); geoopt is
    not installed anywhere this project builds or runs, that could not be verified and is not reproduced;
  * `StfTKConv2dC.reset_parameters` projects the freshly initialised factors onto the manifold; the reference leaves
    them off it (and the layer clamps a table rank above its channel count, see stf_layers).
`RiemannianAdam` is not provided.
"""
from __future__ import annotations

from typing import List

import torch

from . import ops
from ._cabi import TadmmError

_HYPER = ("lr", "momentum", "dampening", "weight_decay", "nesterov")


def is_stiefel(p) -> bool:
    return getattr(p, "manifold", None) == "stiefel"


class StiefelSGD(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov))
        for group in self.param_groups:
            for p in group["params"]:
                if is_stiefel(p):
                    ops.stiefel_desc(p.detach())      # shape / dtype / layout refusals, before anything is launched
        self._plans = {}                              # group index -> (key, StiefelPlan, gradient views, param ids)
        self._old_flags = {}                          # param id -> status word of plans since replaced
        self._euclid = None
        self._euclid_key = None

    # ------------------------------------------------------------------ selection
    def stiefel_params(self) -> List[torch.nn.Parameter]:
        """The parameters that take the Riemannian update, in param-group order."""
        return [p for g in self.param_groups for p in g["params"] if is_stiefel(p)]

    def euclidean_params(self) -> List[torch.nn.Parameter]:
        return [p for g in self.param_groups for p in g["params"] if not is_stiefel(p)]

    # ------------------------------------------------------------------ the two updates
    def _inner_sgd(self):
        groups = [(gi, [p for p in g["params"] if not is_stiefel(p)]) for gi, g in enumerate(self.param_groups)]
        groups = [(gi, ps) for gi, ps in groups if ps]
        key = tuple((gi, tuple(id(p) for p in ps)) for gi, ps in groups)
        if key != self._euclid_key:
            self._euclid_key = key
            self._euclid = None
            if groups:
                self._euclid = torch.optim.SGD([{"params": ps} for _, ps in groups], lr=1e-3)
                self._euclid_groups = [gi for gi, _ in groups]
        if self._euclid is not None:
            self._euclid.state = self.state           # one state: state_dict() covers both kinds of parameter
            for ig, gi in zip(self._euclid.param_groups, self._euclid_groups):
                for k in _HYPER:
                    ig[k] = self.param_groups[gi][k]
        return self._euclid

    def _momentum_buffer(self, p, want: bool):
        if not want:
            return None
        buf = self.state[p].get("momentum_buffer")
        if buf is None or buf.shape != p.shape or buf.device != p.device or buf.dtype != p.dtype \
                or buf.stride() != p.stride():
            new = torch.zeros_like(p, memory_format=torch.preserve_format)
            if new.stride() != p.stride():
                new = torch.empty_strided(p.shape, p.stride(), dtype=p.dtype, device=p.device).zero_()
            if buf is not None:
                new.copy_(buf)
            self.state[p]["momentum_buffer"] = buf = new
        return buf

    def _plan(self, gi: int, active, momentum: float):
        ms = [self._momentum_buffer(p, momentum > 0) for p in active]
        key = tuple((id(p), p.data_ptr(), tuple(p.stride()), None if m is None else m.data_ptr())
                    for p, m in zip(active, ms))
        ent = self._plans.get(gi)
        if ent is None or ent[0] != key:
            if ent is not None:                       # the flags are sticky across rebuilds: keep the old plan's words
                for i, pid in enumerate(ent[3]):
                    word = ent[1].status_of(i)
                    self._old_flags[pid] = torch.maximum(self._old_flags[pid], word) if pid in self._old_flags else word
            # gradient storage laid out like its factor: views into one flat buffer (64-byte aligned) for the
            # contiguous factors, a buffer of its own for a strided one
            offs, total = [], 0
            for p in active:
                offs.append(total)
                total += (p.numel() + 15) // 16 * 16 if p.is_contiguous() else 0
            flat = torch.zeros(max(total, 1), dtype=torch.float32, device=active[0].device)
            views = [flat[o:o + p.numel()].view(p.shape) if p.is_contiguous() else
                     torch.empty_strided(p.shape, p.stride(), dtype=p.dtype, device=p.device).zero_()
                     for p, o in zip(active, offs)]
            plan = ops.StiefelPlan([(p.detach(), g, m) for p, g, m in zip(active, views, ms)])
            ent = (key, plan, views, [id(p) for p in active])
            self._plans[gi] = ent
        return ent[1], ent[2]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            active = [p for p in group["params"] if is_stiefel(p) and p.grad is not None]
            if not active:
                continue
            for p in active:
                if not p.is_cuda:
                    raise TadmmError(-1, f"Stiefel factors must live on a HIP device (got {p.device}); "
                                         "there is no CPU path")
                if p.grad.is_sparse:
                    raise TadmmError(-1, "StiefelSGD does not take sparse gradients")
            plan, views = self._plan(gi, active, group["momentum"])
            stage = [(v, p.grad) for p, v in zip(active, views) if p.grad.data_ptr() != v.data_ptr()]
            if stage:
                torch._foreach_copy_([v for v, _ in stage], [g for _, g in stage])
                for p, v in zip(active, views):
                    p.grad = v
            plan.step(group["lr"], group["momentum"], group["dampening"], group["weight_decay"], group["nesterov"])
        inner = self._inner_sgd()
        if inner is not None:
            inner.step()
        return loss

    # ------------------------------------------------------------------ reporting
    def failed(self) -> list:
        """The Stiefel factors whose retraction broke down in some step of this optimiser (they kept X and M; the flags
        survive plan rebuilds):
        their names where the optimiser was given named parameters, else their indices in `stiefel_params()` order.
        One synchronisation."""
        index, names = {}, {}
        k = 0
        for g in self.param_groups:
            pn = g.get("param_names")
            for j, p in enumerate(g["params"]):
                if is_stiefel(p):
                    index[id(p)] = k
                    if pn is not None:
                        names[id(p)] = pn[j]
                    k += 1
        bad = {ids[i] for _, plan, _, ids in self._plans.values() for i in plan.failed()}
        if self._old_flags:
            pids = list(self._old_flags)
            words = torch.cat([self._old_flags[pid] for pid in pids]).cpu().tolist()
            bad |= {pid for pid, w in zip(pids, words) if w}
        return [names.get(pid, index.get(pid)) for pid in sorted(bad, key=lambda pid: index.get(pid, -1))]
