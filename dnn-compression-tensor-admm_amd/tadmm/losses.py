"""The training criterion of the reference's losses.py: `DistillationLoss` around a base criterion, computed natively.

    criterion = DistillationLoss(base_criterion, teacher_model, distillation_type, alpha, tau)
    loss = criterion(samples, outputs, targets)                  # engines.py:285

`outputs` is a tensor or the tuple (outputs, outputs_kd) of a model with a distillation token; the teacher runs under
`torch.no_grad()`.  The base criterion, the distillation term ('soft': KL at temperature tau, 'hard': cross entropy
against the teacher's argmax) and the gradients of both logit tensors come from one call of csrc/distill.hip (two
launches; `functional.distillation_loss`) when the base criterion is one this module recognises:

  * `torch.nn.CrossEntropyLoss` with `weight=None` and `reduction='mean'`: integer or probability targets, any
    `label_smoothing`, its `ignore_index`;
  * `LabelSmoothingCrossEntropy(smoothing)` and `SoftTargetCrossEntropy()` below, which carry the formulas of the two
    timm classes engines.py:183-189 uses;
  * any object whose class is named like one of the three and carries the same attributes (timm's own classes).

Any other criterion (class weights, another reduction, a user's own module) is called as it is, and only the
distillation term goes through the kernel.  Where the measured rule `ops.distill_loss_pays` says the launch is not ahead,
the same value is composed from torch operations (`functional.distillation_loss_composed`).

Kept from the reference: the constructor's signature and its assertion on the type string, the ValueError when
distillation is on and `outputs` is neither a tensor nor a tuple, and the order of evaluation (base criterion, then the
teacher).

Deliberate differences:
  * the returned loss is a float32 0-dim tensor whatever the logits' type.  The reference under autocast returns the
    same; for pure bfloat16 / float16 logits without autocast torch would return that 16-bit type;
  * an integer label outside [0, C) other than `ignore_index` is dropped from the base term and its denominator and
    counted on the device (`bad_labels()` reads the counter of the latest call) instead of faulting the device;
  * logits and targets must be HIP tensors, the logits of one type (float32, bfloat16 or float16) on one device;
    anything else raises `TadmmError` naming the tensor.  There is no CPU path.

`TinyBertLayerLoss` (below) is the intermediate-layer step of xcompression/task_distill.py:810-828: the attention and
hidden-state MSE terms of every pair and the students' gradients from one call of csrc/layermse.hip.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import functional as HF
from ._cabi import TadmmError


class LabelSmoothingCrossEntropy(torch.nn.Module):
    """NLL loss with label smoothing: (1 - smoothing) * nll + smoothing * mean_c(-log_softmax), mean over the batch."""

    def __init__(self, smoothing: float = 0.1):
        super().__init__()
        assert smoothing < 1.0
        self.smoothing = smoothing
        self.confidence = 1.0 - smoothing

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        logprobs = F.log_softmax(x, dim=-1)
        nll = -logprobs.gather(dim=-1, index=target.unsqueeze(1)).squeeze(1)
        return (self.confidence * nll + self.smoothing * -logprobs.mean(dim=-1)).mean()


class SoftTargetCrossEntropy(torch.nn.Module):
    """Cross entropy against rows of probabilities: sum_c(-target * log_softmax), mean over the batch."""

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return torch.sum(-target * F.log_softmax(x, dim=-1), dim=-1).mean()


def recognise(criterion):
    """What the kernel needs to know of a base criterion: (kind, smoothing, ignore_index) with kind "index", "dense" or
    "by_target" (a CrossEntropyLoss: integer targets are "index", floating ones "dense"), or None for a criterion that
    has to be called as it is.  Decided by the class name and the attributes, so timm's classes are recognised too."""
    name = type(criterion).__name__
    if name == "CrossEntropyLoss":
        if not all(hasattr(criterion, a) for a in ("weight", "reduction", "ignore_index")):
            return None
        if criterion.weight is not None or criterion.reduction != "mean":
            return None
        return "by_target", float(getattr(criterion, "label_smoothing", 0.0)), int(criterion.ignore_index)
    if name == "LabelSmoothingCrossEntropy" and hasattr(criterion, "smoothing"):
        return "index", float(criterion.smoothing), None
    if name == "SoftTargetCrossEntropy":
        return "dense", 0.0, None
    return None


class DistillationLoss(torch.nn.Module):
    """losses.py: DistillationLoss -- a standard criterion plus a knowledge-distillation term from a teacher model's
    prediction (see the module docstring for what is native and what differs)."""

    def __init__(self, base_criterion: torch.nn.Module, teacher_model: torch.nn.Module, distillation_type: str,
                 alpha: float, tau: float):
        super().__init__()
        self.base_criterion = base_criterion
        self.teacher_model = teacher_model
        assert distillation_type in ['none', 'soft', 'hard']
        self.distillation_type = distillation_type
        self.alpha = alpha
        self.tau = tau
        self._counts = None

    def bad_labels(self) -> int:
        """Integer labels of the latest call that were neither `ignore_index` nor inside [0, C).  Reads the device
        counter (one synchronising copy); 0 before the first call and for criteria called as they are."""
        return 0 if self._counts is None else int(self._counts[1])

    def forward(self, inputs, outputs, labels):
        outputs_kd = None
        if isinstance(outputs, torch.Tensor):
            outputs_kd = outputs
        elif isinstance(outputs, tuple):
            outputs, outputs_kd = outputs
        kd = self.distillation_type
        rec = recognise(self.base_criterion)
        box = []
        self._counts = None
        if rec is not None:
            for name, t in (("outputs", outputs), ("labels", labels)):
                if not isinstance(t, torch.Tensor) or not t.is_cuda:
                    where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
                    raise TadmmError(-1, f"DistillationLoss: {name} must live on a HIP device (got {where}); there is no "
                                         "CPU path")
            kind, smoothing, ignore_index = rec
            if kind == "by_target":
                kind = "dense" if labels.dtype.is_floating_point else "index"
        if kd == 'none':
            if rec is None:
                return self.base_criterion(outputs, labels)
            loss = HF.distillation_loss(outputs, None, None, labels, base=kind, kd="none", smoothing=smoothing,
                                        ignore_index=ignore_index, counts=box)
            self._counts = box[0] if box else None
            return loss
        base_loss = None if rec is not None else self.base_criterion(outputs, labels)
        if outputs_kd is None:
            raise ValueError("When knowledge distillation is enabled, the model is "
                             "expected to return a Tuple[Tensor, Tensor] with the output of the "
                             "class_token and the dist_token")
        # don't backprop through the teacher
        with torch.no_grad():
            teacher_outputs = self.teacher_model(inputs)
        if rec is None:
            # the criterion as it is; the kernel returns alpha * kd
            return base_loss * (1 - self.alpha) + HF.distillation_loss(None, outputs_kd, teacher_outputs, None, base="none",
                                                                       kd=kd, alpha=self.alpha, tau=self.tau)
        loss = HF.distillation_loss(outputs, outputs_kd, teacher_outputs, labels, base=kind, kd=kd, alpha=self.alpha,
                                    tau=self.tau, smoothing=smoothing, ignore_index=ignore_index, counts=box)
        self._counts = box[0] if box else None
        return loss


class TinyBertLayerLoss(torch.nn.Module):
    """The intermediate-layer distillation step of xcompression/task_distill.py:810-828 (and task_distill2.py,
    general_distill.py:438-451) as a criterion:

        criterion = TinyBertLayerLoss()
        att_loss, rep_loss = criterion(student_atts[-1], teacher_atts[-1], student_reps[-1], teacher_reps[-1])

    att_loss regresses the students' raw attention scores on the teachers' with every entry <= `threshold` (the additive
    -10000 of masked keys) set to zero on both sides, rep_loss the hidden states; each argument is a tensor or a
    sequence of tensors paired by position.  reduction "batch_sum" is the reference's loop over the batch axis of the
    last layer (sum over samples of the sample's mean), "mean" is MSELoss over each whole tensor, summed over the pairs
    (upstream TinyBERT's loop over layers; `att_weights` / `rep_weights` of the call carry task_distill1.py's per-layer
    scale).  Both losses, and the gradients of every student tensor, come from one call of csrc/layermse.hip (two
    launches; `functional.intermediate_distillation_loss`); `route` ("launch", "composed" or None for the measured rule
    `ops.layer_mse_pays`) is an attribute like that of the BERT modules.  Which teacher layer is paired with which
    student layer stays the caller's business, as in the reference.  Both results are float32 0-dim tensors."""

    def __init__(self, threshold=-1e2, reduction: str = "batch_sum"):
        super().__init__()
        if reduction not in HF.LAYER_MSE_REDUCTIONS:
            raise ValueError(f"TinyBertLayerLoss: reduction is one of {HF.LAYER_MSE_REDUCTIONS} (got {reduction!r})")
        self.threshold = threshold
        self.reduction = reduction
        self.route = None

    def forward(self, student_atts, teacher_atts, student_reps, teacher_reps, att_weights=None, rep_weights=None):
        return HF.intermediate_distillation_loss(student_atts, teacher_atts, student_reps, teacher_reps,
                                                 threshold=self.threshold, reduction=self.reduction,
                                                 att_weights=att_weights, rep_weights=rep_weights, route=self.route)
