"""BertAdam and its learning-rate schedules: what every training script of the reference's BERT sub-project steps with
(`xcompression/transformer/optimization.py`; constructed at task_distill.py:767 and general_distill.py:380).  Swap the
import, keep the call site.

`BertAdam(params, lr, warmup=-1, t_total=-1, schedule='warmup_linear', b1=0.9, b2=0.999, e=1e-6, weight_decay=0.01,
max_grad_norm=1.0)` is a `torch.optim.Optimizer` with the reference's rule, per tensor with a gradient:

        c = min(1, max_grad_norm / (||g|| + 1e-6))        (max_grad_norm > 0, else c = 1: each tensor clipped on its own)
        m <- b1 m + (1 - b1) c g;   v <- b2 v + (1 - b2) (c g)^2                              (no bias correction)
        p <- p - lr * schedule(step) * (m / (sqrt(v) + e) + weight_decay p);   step <- step + 1

  * the float32 dense-contiguous device tensors of a param group go through TWO native launches together (csrc/bertadam.hip,
    `ops.BertAdamPlan`; one launch without clipping), however many there are; the reference's loop costs about twenty
    launches per tensor, and a factorised BERT has a few hundred small tensors;
  * everything else (other dtypes, non-contiguous parameters, CPU tensors) takes `ops.bert_adam_composed`, the same
    arithmetic on `torch._foreach_*` calls in the tensors' own dtype;
  * the schedule multiplier is evaluated on the host at `state['step']` BEFORE the increment and reaches the kernel as
    the scalar lr, so under warm-up the first step moves nothing but still updates m and v (as in the reference);
  * the tensors of a group that have a gradient are partitioned by their step counter; normally that is one class and
    hence one plan.  A tensor without a gradient is left entirely alone: value, state and counter;
  * a plan owns a flat gradient buffer; a step stages the gradients into it with one `_foreach_copy_` and leaves `.grad`
    pointing at the views, so gradients that are zeroed in place (`zero_grad(set_to_none=False)`) accumulate there
    directly and nothing is staged.  A plan is rebuilt when its set of tensors, a storage or a state tensor changes
    (that costs one table upload);
  * `step()` never synchronises;
  * state keys are the reference's: `step` (Python int), `next_m`, `next_v`; `get_lr()` is the reference's, `[0]` before
    the first step included.  A checkpoint written by the reference loads here and one written here loads there.

Differences from the reference, all deliberate:
  * gradients are NOT written back: the reference clips `.grad` in place (`clip_grad_norm_`), this leaves it as it was,
    on both routes.  Every reference script zeroes the gradients right after `step()`, and a write-back would cost one
    more pass over every tensor;
  * the native route takes the norm in float64 and rounds c to float32 once; the reference computes norm and c in float32;
  * `torch.optim.AdamW` (fused or foreach) cannot stand in: it has bias correction, puts eps inside the bias-corrected
    denominator, clips nothing and knows no per-tensor schedule.

The schedule classes (`ConstantLR`, `WarmupConstantSchedule`, `WarmupLinearSchedule`, `WarmupCosineSchedule`,
`WarmupCosineWithHardRestartsSchedule`, `WarmupCosineWithWarmupRestartsSchedule`, `SCHEDULES`) are host code and return the
reference's multipliers, the warning when training runs beyond `t_total` included.
"""
from __future__ import annotations

import abc
import logging
import math

import torch
from torch.optim.optimizer import required

from . import ops

logger = logging.getLogger(__name__)


class _LRSchedule(abc.ABC):
    """A multiplier of the learning rate as a function of progress = step / t_total; `warmup` is the fraction of
    `t_total` over which the multiplier ramps up linearly from 0.  `t_total < 0` switches the schedule off (1 always)."""
    warn_t_total = False            # True where running beyond t_total makes no sense: get_lr warns then

    def __init__(self, warmup=0.002, t_total=-1, **kw):
        super().__init__(**kw)
        if t_total < 0:
            logger.warning("t_total value of {} results in schedule not being applied".format(t_total))
        if warmup != -1 and not 0.0 <= warmup < 1.0:
            raise ValueError("Invalid warmup: {} - should be in [0.0, 1.0[ or -1".format(warmup))
        self.warmup = float(max(warmup, 0.))
        self.t_total = float(t_total)
        self.warned_for_t_total_at_progress = -1

    def get_lr(self, step, nowarn=False):
        """The multiplier at `step`; `nowarn` suppresses the warning about training beyond `t_total`."""
        if self.t_total < 0:
            return 1.
        progress = float(step) / self.t_total
        mult = self.get_lr_(progress)
        if self.warn_t_total and not nowarn and progress > 1. and progress > self.warned_for_t_total_at_progress:
            logger.warning("Training beyond specified 't_total'. Learning rate multiplier set to {}. Please set "
                           "'t_total' of {} correctly.".format(mult, type(self).__name__))
            self.warned_for_t_total_at_progress = progress
        return mult

    @abc.abstractmethod
    def get_lr_(self, progress):
        """The multiplier at `progress` (0 .. 1, beyond 1 when training runs past t_total)."""
        return 1.

    def _after_warmup(self, progress):
        return (progress - self.warmup) / (1 - self.warmup)


class ConstantLR(_LRSchedule):
    def get_lr_(self, progress):
        return 1.


class WarmupConstantSchedule(_LRSchedule):
    """Linear ramp 0 -> 1 over the warm-up, then 1."""
    def get_lr_(self, progress):
        return progress / self.warmup if progress < self.warmup else 1.


class WarmupLinearSchedule(_LRSchedule):
    """Linear ramp 0 -> 1 over the warm-up, then linearly down to 0 at progress 1 (and 0 beyond)."""
    warn_t_total = True

    def get_lr_(self, progress):
        if progress < self.warmup:
            return progress / self.warmup
        return max((progress - 1.) / (self.warmup - 1.), 0.)


class WarmupCosineSchedule(_LRSchedule):
    """Linear ramp over the warm-up, then 0.5 (1 + cos(2 pi cycles x)) over the rest x in [0, 1]: with the default
    cycles = 0.5 half a cosine from 1 down to 0."""
    warn_t_total = True

    def __init__(self, warmup=0.002, t_total=-1, cycles=.5, **kw):
        super().__init__(warmup=warmup, t_total=t_total, **kw)
        self.cycles = cycles

    def get_lr_(self, progress):
        if progress < self.warmup:
            return progress / self.warmup
        return 0.5 * (1. + math.cos(math.pi * self.cycles * 2 * self._after_warmup(progress)))


class WarmupCosineWithHardRestartsSchedule(WarmupCosineSchedule):
    """Linear ramp over the warm-up, then `cycles` half cosines from 1 down to 0, each restarting at 1."""
    def __init__(self, warmup=0.002, t_total=-1, cycles=1., **kw):
        super().__init__(warmup=warmup, t_total=t_total, cycles=cycles, **kw)
        assert cycles >= 1.

    def get_lr_(self, progress):
        if progress < self.warmup:
            return progress / self.warmup
        return 0.5 * (1. + math.cos(math.pi * ((self.cycles * self._after_warmup(progress)) % 1)))


class WarmupCosineWithWarmupRestartsSchedule(WarmupCosineWithHardRestartsSchedule):
    """`cycles` equal parts, each with its own linear ramp over the first `warmup` fraction of the part and a half cosine
    down to 0 over the rest."""
    def __init__(self, warmup=0.002, t_total=-1, cycles=1., **kw):
        assert warmup * cycles < 1.
        super().__init__(warmup=warmup * cycles if warmup >= 0 else warmup, t_total=t_total, cycles=cycles, **kw)

    def get_lr_(self, progress):
        progress = progress * self.cycles % 1.
        if progress < self.warmup:
            return progress / self.warmup
        return 0.5 * (1. + math.cos(math.pi * self._after_warmup(progress)))


SCHEDULES = {
    None: ConstantLR,
    "none": ConstantLR,
    "warmup_cosine": WarmupCosineSchedule,
    "warmup_constant": WarmupConstantSchedule,
    "warmup_linear": WarmupLinearSchedule,
}


class BertAdam(torch.optim.Optimizer):
    """The reference's BertAdam (module docstring): `warmup` is the fraction of `t_total` used for warm-up (-1: none),
    `t_total` the planned number of steps (-1: constant rate), `schedule` a key of `SCHEDULES` or an `_LRSchedule`
    object, `max_grad_norm` the per-tensor clipping norm (-1: no clipping)."""

    def __init__(self, params, lr=required, warmup=-1, t_total=-1, schedule='warmup_linear', b1=0.9, b2=0.999, e=1e-6,
                 weight_decay=0.01, max_grad_norm=1.0, **kwargs):
        if lr is not required and lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not isinstance(schedule, _LRSchedule) and schedule not in SCHEDULES:
            raise ValueError("Invalid schedule parameter: {}".format(schedule))
        if not 0.0 <= b1 < 1.0:
            raise ValueError("Invalid b1 parameter: {} - should be in [0.0, 1.0[".format(b1))
        if not 0.0 <= b2 < 1.0:
            raise ValueError("Invalid b2 parameter: {} - should be in [0.0, 1.0[".format(b2))
        if not e >= 0.0:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(e))
        if isinstance(schedule, _LRSchedule):
            if warmup != -1 or t_total != -1:
                logger.warning("warmup and t_total on the optimizer are ineffective when _LRSchedule object is provided "
                               "as schedule. Please specify custom warmup and t_total in _LRSchedule object.")
        else:
            schedule = SCHEDULES[schedule](warmup=warmup, t_total=t_total)
        super().__init__(params, dict(lr=lr, schedule=schedule, b1=b1, b2=b2, e=e, weight_decay=weight_decay,
                                      max_grad_norm=max_grad_norm))
        self._plans = {}            # group index -> {ids of the plan's tensors: (key, BertAdamPlan, gradient views)}

    def get_lr(self):
        lr = []
        for group in self.param_groups:
            for p in group['params']:
                state = self.state[p]
                if len(state) == 0:
                    return [0]
                lr.append(group['lr'] * group['schedule'].get_lr(state['step']))
        return lr

    # ------------------------------------------------------------------ the native route
    def _key(self, members):
        """What a plan points at beside its own gradient buffer."""
        state = self.state
        return [(p.data_ptr(), state[p]['next_m'].data_ptr(), state[p]['next_v'].data_ptr()) for p in members]

    def _plan(self, gi: int, members):
        """The plan of `members` (parameters of group gi that step together), rebuilt when a storage or a state tensor
        changed; returns (plan, gradient views)."""
        ids = tuple(id(p) for p in members)
        ent = self._plans.setdefault(gi, {}).get(ids)
        if ent is None or ent[0] != self._key(members):
            # gradient storage: views into one flat buffer, each 64-byte aligned
            offs, total = [], 0
            for p in members:
                offs.append(total)
                total += (p.numel() + 15) // 16 * 16
            flat = torch.zeros(total, dtype=torch.float32, device=members[0].device)
            views = [flat[o:o + p.numel()].view(p.shape) for p, o in zip(members, offs)]
            plan = ops.BertAdamPlan([(p.detach(), g, self.state[p]['next_m'], self.state[p]['next_v'])
                                     for p, g in zip(members, views)])
            ent = (self._key(members), plan, views)
            self._plans[gi][ids] = ent
        return ent[1], ent[2]

    @staticmethod
    def _stage(members, views):
        stage = [(v, p.grad) for p, v in zip(members, views) if p.grad.data_ptr() != v.data_ptr()]
        if stage:
            torch._foreach_copy_([v for v, _ in stage], [g for _, g in stage])
            for p, v in zip(members, views):
                p.grad = v

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            classes = {}                                  # step counter -> the group's tensors standing at it
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError('Adam does not support sparse gradients, please consider SparseAdam instead')
                state = self.state[p]
                if len(state) == 0:
                    state['step'] = 0
                    state['next_m'] = torch.zeros_like(p.data)
                    state['next_v'] = torch.zeros_like(p.data)
                classes.setdefault(state['step'], []).append(p)
            used = set()
            for count, members in classes.items():
                lr = group['lr'] * group['schedule'].get_lr(count)
                hyper = (lr, group['b1'], group['b2'], group['e'], group['weight_decay'], group['max_grad_norm'])
                # the usual step: the class is one plan's tensors, nothing moved, and every .grad still is that plan's
                # view (so it is float32, dense and staged): no per-tensor checks, straight to the two launches
                ids = tuple(id(p) for p in members)
                ent = self._plans.get(gi, {}).get(ids)
                if ent is not None and all(p.grad is v for p, v in zip(members, ent[2])) and ent[0] == self._key(members):
                    used.add(ids)
                    ent[1].step(*hyper)
                    for p in members:
                        self.state[p]['step'] += 1
                    continue
                native = [p for p in members
                          if ops.bert_adam_native(p, p.grad, self.state[p]['next_m'], self.state[p]['next_v'])]
                if native:
                    # (one plan per device: a group normally lives on one)
                    for dev in dict.fromkeys(p.device for p in native):
                        part = [p for p in native if p.device == dev]
                        plan, views = self._plan(gi, part)
                        used.add(tuple(id(p) for p in part))
                        self._stage(part, views)
                        plan.step(*hyper)
                taken = set(id(p) for p in native)
                rest = [p for p in members if id(p) not in taken]
                if rest:
                    ops.bert_adam_composed(rest, [p.grad for p in rest], [self.state[p]['next_m'] for p in rest],
                                           [self.state[p]['next_v'] for p in rest], *hyper)
                for p in members:
                    self.state[p]['step'] += 1
            if gi in self._plans:                         # plans of member sets that no longer step together
                self._plans[gi] = {ids: ent for ids, ent in self._plans[gi].items() if ids in used}
        return loss
