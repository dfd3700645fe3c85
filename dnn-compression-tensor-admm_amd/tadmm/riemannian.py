"""Riemannian optimisers for models with Stiefel factors (`StfTKConv2dC`): what the reference gets from
`geoopt.optim.RiemannianSGD` and, with `--opt adam`, `geoopt.optim.RiemannianAdam` for every model whose name starts
with `stf` (engines.py:167-174).

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

`StiefelAdam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, stabilize=None)` is the Adam
counterpart, built on the same plans, gradient staging and failure flags (`_StiefelOptimizer`):

  * per factor, in the same single launch per param group (`ops.StiefelPlan.adam_step`), with t the factor's counter:
        t <- t + 1;   g, r as above;   s = sum r^2
        M <- beta1 M + (1 - beta1) r;   v <- beta2 v + (1 - beta2) s;   u = amsgrad ? (vmax <- max(vmax, v)) : v
        X <- qr(X - lr / ((1 - beta1^t) (sqrt(u / (1 - beta2^t)) + eps)) M).Q;   M <- M - X sym(X^T M)
    the second moment is ONE number per factor (the squared tangent norm), as geoopt's Stiefel manifold has it;
  * `state[p]` of a factor holds `exp_avg` (laid out like the factor), `exp_avg_sq` (float32), `step` (int32) and with
    amsgrad `max_exp_avg_sq`: one-element device tensors, views of per-group flat arrays that the launch updates, so
    the bias corrections are computed on the device and `step()` never synchronises.  `state_dict()` /
    `load_state_dict()` round-trip them; a change of the set of factors with a gradient, a replaced buffer or a loaded
    state rebuilds the plan and carries every factor's state over;
  * all other parameters take an inner `torch.optim.Adam` with the group's hyper-parameters, sharing this optimiser's state;
  * a factor that failed, or had no gradient, keeps X, `exp_avg`, `exp_avg_sq`, `max_exp_avg_sq` and `step`;
  * `stabilize` is accepted for call-site compatibility and ignored: every step re-orthonormalises in fp64, so there
    is nothing left to stabilise.  `maximize`, `foreach`, `capturable` and `fused` are not offered.

Differences from geoopt, all deliberate:
  * the momentum buffer of `StiefelSGD` starts at ZERO, so the first step moves along (1 - dampening) r.  geoopt seeds
    the buffer differently on its first step (from memory of its source: with the gradient itself, like torch's SGD);
    geoopt is not installed anywhere this project builds or runs, that could not be verified and is not reproduced;
  * `StfTKConv2dC.reset_parameters` projects the freshly initialised factors onto the manifold; the reference leaves
    them off it (and the layer clamps a table rank above its channel count, see stf_layers);
  * `StiefelAdam` counts steps per factor (geoopt: one counter per param group), so a skipped or failed factor does
    not advance its bias correction; the two agree whenever every factor has a gradient at every step;
  * `StiefelAdam` stores `exp_avg_sq` as one number per factor, not as a buffer of the factor's shape holding that
    number everywhere (from memory of geoopt's source, unverified: its Stiefel manifold has no `component_inner` of
    its own, so the base class's `inner(..., keepdim=True)` is broadcast).
"""
from __future__ import annotations

from typing import List

import torch

from . import ops
from ._cabi import TadmmError


def is_stiefel(p) -> bool:
    return getattr(p, "manifold", None) == "stiefel"


class _StiefelOptimizer(torch.optim.Optimizer):
    """What `StiefelSGD` and `StiefelAdam` share: the Stiefel / Euclidean selection, one `ops.StiefelPlan` per param
    group keyed by what its descriptors point at, the flat gradient buffer with `.grad` views, the inner torch
    optimiser of the Euclidean parameters, and failure flags that survive plan rebuilds.  A subclass names its inner
    optimiser (`_INNER`, `_HYPER`), its per-factor buffer (`_BUFFER`) and, where it keeps more per-factor state than
    that buffer, `_state_key` / `_rebind_state`."""
    _INNER = None
    _HYPER = ()
    _BUFFER = None

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
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
    def _inner(self):
        groups = [(gi, [p for p in g["params"] if not is_stiefel(p)]) for gi, g in enumerate(self.param_groups)]
        groups = [(gi, ps) for gi, ps in groups if ps]
        key = tuple((gi, tuple(id(p) for p in ps)) for gi, ps in groups)
        if key != self._euclid_key:
            self._euclid_key = key
            self._euclid = None
            if groups:
                self._euclid = self._INNER([{"params": ps} for _, ps in groups], lr=1e-3)
                self._euclid_groups = [gi for gi, _ in groups]
        if self._euclid is not None:
            self._euclid.state = self.state           # one state: state_dict() covers both kinds of parameter
            for ig, gi in zip(self._euclid.param_groups, self._euclid_groups):
                for k in self._HYPER:
                    ig[k] = self.param_groups[gi][k]
        return self._euclid

    def _buffer(self, p, want: bool):
        """The factor's `_BUFFER` entry of the state (momentum), laid out like the factor; created at zero."""
        if not want:
            return None
        buf = self.state[p].get(self._BUFFER)
        if buf is None or buf.shape != p.shape or buf.device != p.device or buf.dtype != p.dtype \
                or buf.stride() != p.stride():
            new = torch.zeros_like(p, memory_format=torch.preserve_format)
            if new.stride() != p.stride():
                new = torch.empty_strided(p.shape, p.stride(), dtype=p.dtype, device=p.device).zero_()
            if buf is not None:
                new.copy_(buf)
            self.state[p][self._BUFFER] = buf = new
        return buf

    def _state_key(self, gi: int, active) -> tuple:
        """What else, beside the factors and their buffers, a group's plan depends on."""
        return ()

    def _rebind_state(self, gi: int, active, plan) -> None:
        """Called after a group's plan was rebuilt, before its key is taken."""

    def _plan(self, gi: int, active, want_buffer: bool):
        ms = [self._buffer(p, want_buffer) for p in active]

        def key():
            return tuple((id(p), p.data_ptr(), tuple(p.stride()), None if m is None else m.data_ptr())
                         for p, m in zip(active, ms)) + self._state_key(gi, active)

        ent = self._plans.get(gi)
        if ent is None or ent[0] != key():
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
            self._rebind_state(gi, active, plan)
            ent = (key(), plan, views, [id(p) for p in active])
            self._plans[gi] = ent
        return ent[1], ent[2]

    def _active(self, group):
        """The group's factors with a gradient, refused where there is no route for them."""
        active = [p for p in group["params"] if is_stiefel(p) and p.grad is not None]
        for p in active:
            if not p.is_cuda:
                raise TadmmError(-1, f"Stiefel factors must live on a HIP device (got {p.device}); "
                                     "there is no CPU path")
            if p.grad.is_sparse:
                raise TadmmError(-1, f"{type(self).__name__} does not take sparse gradients")
        return active

    @staticmethod
    def _stage(active, views):
        stage = [(v, p.grad) for p, v in zip(active, views) if p.grad.data_ptr() != v.data_ptr()]
        if stage:
            torch._foreach_copy_([v for v, _ in stage], [g for _, g in stage])
            for p, v in zip(active, views):
                p.grad = v

    def _step_group(self, gi: int, group, active) -> None:
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            active = self._active(group)
            if active:
                self._step_group(gi, group, active)
        inner = self._inner()
        if inner is not None:
            inner.step()
        return loss

    # ------------------------------------------------------------------ reporting
    def failed(self) -> list:
        """The Stiefel factors whose retraction broke down in some step of this optimiser (they kept X and their state;
        the flags survive plan rebuilds):
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


class StiefelSGD(_StiefelOptimizer):
    _INNER = torch.optim.SGD
    _HYPER = ("lr", "momentum", "dampening", "weight_decay", "nesterov")
    _BUFFER = "momentum_buffer"

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

    def _step_group(self, gi, group, active):
        plan, views = self._plan(gi, active, group["momentum"] > 0)
        self._stage(active, views)
        plan.step(group["lr"], group["momentum"], group["dampening"], group["weight_decay"], group["nesterov"])


class StiefelAdam(_StiefelOptimizer):
    _INNER = torch.optim.Adam
    _HYPER = ("lr", "betas", "eps", "weight_decay", "amsgrad")
    _BUFFER = "exp_avg"
    # the one-element entries of a factor's state and the dtype of the group's flat array behind each
    _SCALARS = (("exp_avg_sq", torch.float32), ("max_exp_avg_sq", torch.float32), ("step", torch.int32))

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, stabilize=None):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        del stabilize                                 # every step re-orthonormalises in fp64 (module docstring)
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                                      amsgrad=bool(amsgrad)))
        self._flat = {}                               # group index -> {state name: flat array in the plan's slot order}

    def _names(self, gi):
        amsgrad = self.param_groups[gi]["amsgrad"]
        return [(k, dt) for k, dt in self._SCALARS if amsgrad or k != "max_exp_avg_sq"]

    def _state_key(self, gi, active):
        # a loaded or replaced state entry no longer points into the group's flat arrays: the plan is rebuilt
        return tuple(None if t is None else t.data_ptr()
                     for p in active for t in (self.state[p].get(k) for k, _ in self._names(gi)))

    def _rebind_state(self, gi, active, plan):
        # one flat array per entry, in the plan's slot order (native factors first); what a factor had is carried over
        dev = active[0].device
        order = [active[i] for i in plan.order]
        flat = {}
        for k, dt in self._names(gi):
            old = [self.state[p].get(k) for p in order]
            flat[k] = torch.cat([torch.zeros(1, dtype=dt, device=dev) if t is None else
                                 t.detach().to(device=dev, dtype=dt).reshape(1) for t in old])
            for slot, p in enumerate(order):
                self.state[p][k] = flat[k][slot:slot + 1]
        self._flat[gi] = flat

    def _step_group(self, gi, group, active):
        plan, views = self._plan(gi, active, True)
        self._stage(active, views)
        flat = self._flat[gi]
        plan.adam_step(group["lr"], group["betas"], group["eps"], group["weight_decay"], group["amsgrad"],
                       flat["exp_avg_sq"], flat.get("max_exp_avg_sq"), flat["step"])
