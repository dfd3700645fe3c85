"""CPU-only checks of Riemannian Adam on Stiefel factors: properties of the float64 yardstick of the GPU tests
(tests/_stiefel_adam_ref.py), the refusals `StiefelAdam` raises before any launch, its selection of parameters, and the
C entry's answer to a null plan."""
import ctypes as C

import numpy as np
import pytest
import torch

import _stiefel_adam_ref as A

SHAPES = [(3, 1), (16, 16), (33, 7), (64, 64)]


class HP:
    ranks = {"k": [6, 5]}


def _draw(n, p, seed):
    rng = np.random.default_rng(seed)
    x = A.qr_pos(rng.standard_normal((n, p)))
    g = rng.standard_normal((n, p))
    m = A.tangent(x, rng.standard_normal((n, p)))
    return x, g, m


@pytest.mark.parametrize("n,p", SHAPES)
@pytest.mark.parametrize("amsgrad", [False, True])
def test_reference_step_stays_on_the_manifold_and_transports(n, p, amsgrad):
    x, g, m = _draw(n, p, 100 * n + p)
    xn, mn, v, vmax, t = A.step(x, g, m, 0.3, 0.7, 3, 0.05, (0.9, 0.999), 1e-8, 0.05, amsgrad)
    assert A.orth_error(xn) <= 1e-14
    assert np.abs(A.sym(xn.T @ mn)).max() <= 1e-13 * max(1.0, np.abs(mn).max())        # tangent at X+
    assert t == 4 and v > 0 and vmax == (max(0.7, v) if amsgrad else 0.7)
    # the float32 restatement is the same algorithm: it agrees to single precision
    x32, m32, v32, _, t32 = A.step_f32(x.astype(np.float32), g.astype(np.float32), m.astype(np.float32), 0.3, 0.7, 3, 0.05,
                                       (0.9, 0.999), 1e-8, 0.05, amsgrad)
    assert t32 == 4 and np.abs(x32 - xn).max() <= 1e-5 * np.abs(xn).max() and abs(v32 - v) <= 1e-5 * v
    assert np.abs(m32 - mn).max() <= 1e-5 * np.abs(mn).max()


@pytest.mark.parametrize("n,p", SHAPES)
def test_first_step_from_zero_state_has_unit_direction(n, p):
    """t = 1, M = 0, v = 0: M' = (1 - b1) r, c1 = 1 - b1, v' / c2 = ||r||^2, so Y - X = -lr r / (||r|| + eps)."""
    x, g, _ = _draw(n, p, 7 * n + p)
    lr, eps = 0.05, 1e-3
    y, m, v, u, t = A.pre_retraction(x, g, np.zeros_like(x), 0.0, 0.0, 0, lr, (0.9, 0.999), eps)
    r = np.linalg.norm(A.tangent(x, g))
    assert t == 1 and u == v
    assert abs(np.linalg.norm(y - x) - lr * r / (r + eps)) <= 1e-12


@pytest.mark.parametrize("n,p", SHAPES)
def test_zero_gradient_from_zero_state_stays_put(n, p):
    x, _, _ = _draw(n, p, 3 * n + p)
    z = np.zeros_like(x)
    xn, mn, v, vmax, t = A.step(x, z, z, 0.0, 0.0, 0, 0.05)
    assert np.isfinite(xn).all() and np.isfinite(mn).all()
    assert np.abs(xn - x).max() <= 1e-14 and v == 0.0 and t == 1 and not mn.any()


def test_constructor_refusals():
    from tadmm import riemannian, stf_layers
    from tadmm._cabi import TadmmError
    p = [torch.nn.Parameter(torch.zeros(3))]
    for kw, word in ((dict(lr=-1.0), "learning rate"), (dict(eps=-1e-8), "epsilon"),
                     (dict(betas=(1.0, 0.999)), "beta parameter at index 0"),
                     (dict(betas=(0.9, -0.1)), "beta parameter at index 1"),
                     (dict(weight_decay=-1.0), "weight_decay")):
        with pytest.raises(ValueError, match=word):
            riemannian.StiefelAdam(p, **kw)
    for kw in (dict(maximize=True), dict(foreach=True), dict(capturable=True), dict(fused=True)):
        with pytest.raises(TypeError):
            riemannian.StiefelAdam(p, **kw)
    with pytest.raises(TadmmError, match="n >= p"):                 # more columns than rows: before anything is launched
        riemannian.StiefelAdam([stf_layers.StiefelParameter(torch.zeros(3, 5))])
    riemannian.StiefelAdam(p, stabilize=10)                          # accepted and ignored


def test_selection_defaults_empty_state_and_no_cpu_path():
    import tadmm
    from tadmm import riemannian, stf_layers
    from tadmm._cabi import TadmmError
    assert tadmm.StiefelAdam is riemannian.StiefelAdam
    assert issubclass(riemannian.StiefelAdam, torch.optim.Optimizer)
    assert riemannian.StiefelAdam.__mro__[1] is riemannian.StiefelSGD.__mro__[1]         # the shared base
    m = stf_layers.StfTKConv2dC(12, 16, 3, hp_dict=HP, name="k")
    lin = torch.nn.Linear(4, 3)
    opt = riemannian.StiefelAdam(list(m.parameters()) + list(lin.parameters()))
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["amsgrad"]) == (1e-3, (0.9, 0.999), 1e-8, 0, False)
    assert [id(p) for p in opt.stiefel_params()] == [id(m.first_kernel), id(m.last_kernel)]
    assert [id(p) for p in opt.euclidean_params()] == [id(m.core_kernel), id(m.bias), id(lin.weight), id(lin.bias)]
    assert len(opt.state) == 0 and opt.state_dict()["state"] == {} and opt.failed() == []
    opt.step()                                                          # no gradients anywhere: nothing to do
    assert len(opt.state) == 0
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(TadmmError, match="no CPU path"):
        opt.step()


def test_c_entry_refuses_a_null_plan():
    from tadmm import _cabi
    lib = _cabi.load()
    assert lib.tadmm_stiefel_adam_step(None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, None, None, None, None, None) == -1
