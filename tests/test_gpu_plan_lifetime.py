"""Lifetime of the grouped projection plans through their shared base (`ops._LayerPlan`): close() twice, collection of a
closed plan, a second plan over the same tensors, and a constructor that raised half-way.  The layers are the smallest SVD
layer of test_gpu_projection.py and the smallest 4-D Tucker layer of test_gpu_layers.py."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _layer(kind):
    from tadmm import ops
    from tadmm._cabi import KIND_SVD
    rng = np.random.default_rng(7)
    if kind == "svd":
        w = torch.from_numpy(rng.standard_normal((11, 3)).astype(np.float32)).to(DEV)
        return ops.ProjectionPlan, dict(kind=KIND_SVD, W=w, U=torch.zeros_like(w), Z=torch.empty_like(w), ranks=1)
    w = torch.from_numpy((rng.standard_normal((64, 4, 1, 1)) * 0.3).astype(np.float32)).to(DEV)
    return ops.TuckerPlan, dict(W=w, U=torch.zeros_like(w), Z=torch.empty_like(w), ranks=[8, 3])


@pytest.mark.parametrize("kind", ["svd", "tucker4d"])
def test_close_twice_collect_and_rebuild(kind):
    """update_u=False leaves W and U as they were, so the second plan projects the same input: bitwise the same residual."""
    cls, layer = _layer(kind)
    plan = cls([layer])
    first = plan.run(update_u=False).clone()
    z_first = layer["Z"].clone()
    plan.close()
    plan.close()
    assert plan._plan is None
    del plan
    gc.collect()
    again = cls([layer])
    second = again.run(update_u=False)
    assert torch.equal(first, second) and torch.equal(first.view(torch.int64), second.view(torch.int64))
    assert torch.equal(z_first, layer["Z"])
    assert float(first[0]) > 0
    del again                                             # never closed: the finalizer destroys the native plan
    gc.collect()
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["svd", "tucker4d"])
def test_a_constructor_that_raised_leaves_nothing_behind(kind):
    from tadmm._cabi import TadmmError
    cls, layer = _layer(kind)
    layer["U"] = torch.zeros(layer["W"].numel() + 1, device=DEV)
    plan = cls.__new__(cls)
    with pytest.raises(TadmmError, match="U shape differs from W") as info:
        plan.__init__([layer])
    assert info.value.status == -1
    plan.close()
    plan.close()
    assert plan._plan is None
    del plan
    gc.collect()
    with pytest.raises(TadmmError, match="U shape differs from W"):
        cls([layer])
    gc.collect()
