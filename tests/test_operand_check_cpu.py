"""The one device-operand check of `tadmm.ops` (`_operand`), through every public entry that used to carry a hand-written
copy of it: a CPU tensor is refused with TadmmError, status -1, "there is no CPU path" -- before the library is loaded
for a launch, so no device is needed.  Tensors are (2, 2) or (1, 1, 2, 2); `lstm_planes` checks its (4H, H) shape first
(tests/test_lstm_host_cpu.py pins that order) and gets the smallest weight that passes it, (4, 1)."""
import pytest
import torch

M = torch.zeros(2, 2)                       # a matrix / a stand-in for weight planes (never read: x is refused first)
IMG = torch.zeros(1, 1, 2, 2)               # an NCHW image, and a TT-matrix core (r, n, m, r') with r_0 = 1
G = ((1, 1), (1, 1), (0, 0), (1, 1))        # kernel, stride, padding, dilation


def _entries():
    from tadmm import ops
    bf = M.bfloat16()
    return {
        "mm_nt_bf16": lambda: ops.mm_nt_bf16(bf, bf),
        "wgrad": lambda: ops.wgrad(M, M),
        "wgrad_plan": lambda: ops.wgrad_plan(IMG, IMG),
        "weight_planes": lambda: ops.weight_planes(M, 1),
        "chain_fused": lambda: ops.chain_fused(M, M, M, None, 2),
        "chain_fused_save": lambda: ops.chain_fused_save(M, M, M, None, 2, 1),
        "chain_single": lambda: ops.chain_single(M, M, None, 2),
        "svd_conv": lambda: ops.svd_conv(IMG, M, M, None, 2),
        "svd_conv_save": lambda: ops.svd_conv_save(IMG, M, M, None, 2, 1),
        "conv_chain": lambda: ops.conv_chain(IMG, M, M, M, None, 2, *G),
        "conv_chain_save": lambda: ops.conv_chain_save(IMG, M, M, M, None, 2, 1, 1, *G),
        "conv_chain_bwd": lambda: ops.conv_chain_bwd(IMG, M, M, M, (1, 1, 2, 2), 1, 1, *G),
        "core_conv": lambda: ops.core_conv(IMG, M, 1, (1, 1)),
        "core_conv_dgrad": lambda: ops.core_conv_dgrad(IMG, M, (1, 1, 2, 2), (1, 1)),
        "core_conv_wgrad": lambda: ops.core_conv_wgrad(IMG, IMG, (1, 1)),
        "core_conv_wgrad_plan": lambda: ops.core_conv_wgrad_plan(IMG, IMG, (1, 1)),
        "ttm_gather": lambda: ops.ttm_gather([IMG], M.long()),
        "ttm_gather_bwd": lambda: ops.ttm_gather_bwd([IMG], M.long(), M),
        "lstm_seq": lambda: ops.lstm_seq(M, M),
        "lstm_seq_save": lambda: ops.lstm_seq_save(M, M),
        "lstm_seq_bwd": lambda: ops.lstm_seq_bwd(M, M, M),
        "lstm_planes": lambda: ops.lstm_planes(torch.zeros(4, 1)),
        "gram": lambda: ops.gram(M),
        "ProjectionPlan": lambda: ops.ProjectionPlan([dict(kind=2, W=M, U=M, Z=M, ranks=1)]),
        "TuckerPlan": lambda: ops.TuckerPlan([dict(W=M, U=M, Z=M, ranks=[1, 1])]),
    }


ENTRIES = ["mm_nt_bf16", "wgrad", "wgrad_plan", "weight_planes", "chain_fused", "chain_fused_save", "chain_single",
           "svd_conv", "svd_conv_save", "conv_chain", "conv_chain_save", "conv_chain_bwd", "core_conv", "core_conv_dgrad",
           "core_conv_wgrad", "core_conv_wgrad_plan", "ttm_gather", "ttm_gather_bwd", "lstm_seq", "lstm_seq_save",
           "lstm_seq_bwd", "lstm_planes", "gram", "ProjectionPlan", "TuckerPlan"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_cpu_tensor_is_refused_by_the_operand_check(entry):
    from tadmm._cabi import TadmmError
    with pytest.raises(TadmmError, match="there is no CPU path") as info:
        _entries()[entry]()
    assert info.value.status == -1


def test_every_entry_is_listed():
    assert sorted(_entries()) == sorted(ENTRIES)
