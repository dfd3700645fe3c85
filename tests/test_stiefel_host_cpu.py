"""CPU-only checks of the Stiefel layer and optimiser: constructor shapes and keys, selection, descriptor packing,
refusals raised before any launch, the optimiser's state_dict round trip, the LDS-fit rule, and the float64 yardstick
of the GPU tests itself."""
import ctypes as C

import numpy as np
import pytest
import torch

import _stiefel_ref as R


class HP:
    ranks = {"k": [6, 5]}


def test_constructor_shapes_and_state_dict_keys():
    from tadmm import stf_layers
    m = stf_layers.StfTKConv2dC(12, 16, 3, padding=1, hp_dict=HP, name="k")
    assert list(m.state_dict()) == ["first_kernel", "core_kernel", "last_kernel", "bias"]
    assert m.first_kernel.shape == (12, 5) and m.core_kernel.shape == (6, 5, 3, 3) and m.last_kernel.shape == (16, 6)
    assert m.bias.shape == (16,) and m.in_rank == 5 and m.out_rank == 6
    for p in (m.first_kernel, m.last_kernel):
        assert isinstance(p, stf_layers.StiefelParameter) and isinstance(p, torch.nn.Parameter)
        assert p.manifold == "stiefel" and p.requires_grad
    assert not hasattr(m.core_kernel, "manifold")
    nb = stf_layers.StfTKConv2dC(12, 16, 3, bias=False, hp_dict=HP, name="k")
    assert list(nb.state_dict()) == ["first_kernel", "core_kernel", "last_kernel"] and nb.bias is None
    # the flat alias and the package export name the same class
    import tadmm
    assert tadmm.StfTKConv2dC is stf_layers.StfTKConv2dC and tadmm.StiefelParameter is stf_layers.StiefelParameter
    # a module built without a device waits for one to project its factors; loading a state_dict settles them
    assert m._pending_projection
    m.load_state_dict(nb.state_dict(), strict=False)
    assert not m._pending_projection
    import copy
    assert isinstance(copy.deepcopy(m).first_kernel, stf_layers.StiefelParameter)


def test_rank_above_the_channel_count_is_clamped():
    from tadmm import stf_layers

    class Over:
        ranks = {"k": [24, 20]}                     # tk_resnet32_hp 3x, layer2.0.conv1: 32 x 16 channels

    m = stf_layers.StfTKConv2dC(16, 32, 3, hp_dict=Over, name="k")
    assert m.ranks == [24, 20] and (m.out_rank, m.in_rank) == (24, 16)
    assert m.first_kernel.shape == (16, 16) and m.last_kernel.shape == (32, 24) and m.core_kernel.shape == (24, 16, 3, 3)


def test_constructor_errors_match_the_reference():
    from tadmm import stf_layers
    with pytest.raises(ValueError, match="groups must be 1 in this mode"):
        stf_layers.StfTKConv2dC(12, 16, 3, groups=2, hp_dict=HP, name="k")
    with pytest.raises(ValueError, match="padding_mode must be zero in this mode"):
        stf_layers.StfTKConv2dC(12, 16, 3, padding_mode="reflect", hp_dict=HP, name="k")


def test_optimiser_selects_exactly_the_stiefel_parameters():
    from tadmm import riemannian, stf_layers
    m = stf_layers.StfTKConv2dC(12, 16, 3, hp_dict=HP, name="k")
    lin = torch.nn.Linear(4, 3)
    opt = riemannian.StiefelSGD(list(m.parameters()) + list(lin.parameters()), lr=0.1, momentum=0.9)
    assert [id(p) for p in opt.stiefel_params()] == [id(m.first_kernel), id(m.last_kernel)]
    assert [id(p) for p in opt.euclidean_params()] == [id(m.core_kernel), id(m.bias), id(lin.weight), id(lin.bias)]
    with pytest.raises(ValueError, match="Nesterov"):
        riemannian.StiefelSGD(m.parameters(), lr=0.1, nesterov=True)
    # there is no CPU path: a step on host tensors raises instead of computing something else
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    from tadmm._cabi import TadmmError
    with pytest.raises(TadmmError, match="no CPU path"):
        opt.step()


def test_descriptor_packing_from_a_strided_view():
    from tadmm import _cabi, ops
    buf = torch.zeros(10, 7)
    x, g = buf[:, :4], torch.ones(10, 7)[:, :4]
    d = ops.stiefel_desc(x, g, None)
    assert (d.rows, d.cols, d.ld) == (10, 4, 7)
    assert d.X == x.data_ptr() and d.G == g.data_ptr() and d.M is None
    c = ops.stiefel_desc(torch.zeros(5, 3))
    assert (c.rows, c.cols, c.ld) == (5, 3, 3) and c.G is None
    assert C.sizeof(_cabi.StiefelDesc) == _cabi.load().tadmm_stiefel_desc_bytes() == 40


def test_refusals_before_any_launch():
    from tadmm import ops, riemannian, stf_layers
    from tadmm._cabi import TadmmError
    with pytest.raises(TadmmError, match="n >= p"):
        ops.stiefel_desc(torch.zeros(3, 5))
    with pytest.raises(TadmmError, match="float32"):
        ops.stiefel_desc(torch.zeros(5, 3, dtype=torch.float64))
    with pytest.raises(TadmmError, match="row-major"):
        ops.stiefel_desc(torch.zeros(3, 5).t())
    with pytest.raises(TadmmError, match="row stride"):
        ops.stiefel_desc(torch.zeros(10, 7)[:, :4], torch.zeros(10, 4))           # gradient laid out differently
    with pytest.raises(TadmmError, match="matrix"):
        ops.stiefel_desc(torch.zeros(5, 3, 1))
    with pytest.raises(TadmmError, match="n >= p"):                                  # the optimiser checks at construction
        riemannian.StiefelSGD([stf_layers.StiefelParameter(torch.zeros(3, 5))], lr=0.1)
    with pytest.raises(TadmmError, match="no CPU path"):
        ops.StiefelPlan([(torch.zeros(5, 3), None, None)])


def test_c_entries_refuse_bad_descriptors_and_oversized_factors():
    from tadmm import _cabi
    lib = _cabi.load()
    h = C.c_void_p()
    lib.tadmm_create(0, C.byref(h))          # no GPU here: the handle is still usable for host-side checks
    assert h.value
    size = C.c_size_t()
    ws = C.create_string_buffer(1024)

    def desc(rows, cols, ld, x=4096, g=8192, m=12288):
        d = _cabi.StiefelDesc()
        d.X, d.G, d.M, d.rows, d.cols, d.ld = x, g, m, rows, cols, ld
        return (_cabi.StiefelDesc * 1)(d)

    assert lib.tadmm_stiefel_workspace_bytes(1, desc(64, 64, 64), C.byref(size)) == 0 and size.value >= 40
    plan = C.c_void_p()
    for bad, word in ((desc(3, 5, 5), "rows >= cols"), (desc(5, 3, 2), "ld 2 < cols 3"), (desc(5, 3, 3, x=None), "NULL"),
                      (desc(5, 3, 3, x=4098), "misaligned"), (desc(5, 0, 3), "rows >= cols")):
        assert lib.tadmm_stiefel_workspace_bytes(1, bad, C.byref(size)) == -1
        assert lib.tadmm_stiefel_plan_create(h, 1, bad, ws, 1024, None, C.byref(plan)) == -1 and not plan.value
        assert word in lib.tadmm_last_error(h).decode()
    assert lib.tadmm_stiefel_workspace_bytes(0, desc(5, 3, 3), C.byref(size)) == -1
    assert lib.tadmm_stiefel_plan_create(h, 1, desc(124, 64, 64), ws, 1024, None, C.byref(plan)) == -5
    assert "does not fit" in lib.tadmm_last_error(h).decode() and not plan.value
    assert lib.tadmm_stiefel_step(None, 0.1, 0.0, 0.0, 0.0, 0, None, None) == -1
    lib.tadmm_destroy(h)


def test_lds_fit_rule_is_a_pure_function():
    from tadmm import _cabi, ops
    assert ops.stiefel_fits(64, 64) and ops.stiefel_fits(3, 1) and ops.stiefel_fits(16, 16)
    assert ops.stiefel_lds_bytes(64, 64) == 3 * 64 * 65 * 4 + 2 * 64 * 65 * 8 + 2 * 64 * 8
    assert ops.stiefel_fits(123, 64) and not ops.stiefel_fits(124, 64)             # the bound at 64 columns
    assert ops.stiefel_lds_bytes(123, 64) <= 160 * 1024 < ops.stiefel_lds_bytes(124, 64)
    assert not ops.stiefel_fits(3, 5) and not ops.stiefel_fits(4, 0)
    # the library draws the same line
    lib = _cabi.load()
    size = C.c_size_t()
    for n, p in ((64, 64), (123, 64), (124, 64), (76, 76), (77, 77), (2000, 4), (4000, 4)):
        d = _cabi.StiefelDesc()
        d.X, d.rows, d.cols, d.ld = 4096, n, p, p
        rc = lib.tadmm_stiefel_workspace_bytes(1, (_cabi.StiefelDesc * 1)(d), C.byref(size))
        assert (rc == 0) == ops.stiefel_fits(n, p) and rc in (0, -5), (n, p, rc)


def test_optimiser_state_dict_round_trip():
    from tadmm import riemannian, stf_layers

    def build():
        torch.manual_seed(0)
        m = stf_layers.StfTKConv2dC(12, 16, 3, hp_dict=HP, name="k")
        return m, riemannian.StiefelSGD(m.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)

    m, opt = build()
    g = torch.Generator().manual_seed(1)
    for p in m.parameters():
        opt.state[p]["momentum_buffer"] = torch.randn(p.shape, generator=g)
    sd = opt.state_dict()
    assert len(sd["state"]) == 4 and sd["param_groups"][0]["momentum"] == 0.9
    m2, opt2 = build()
    opt2.load_state_dict(sd)
    for p, q in zip(m.parameters(), m2.parameters()):
        assert torch.equal(opt.state[p]["momentum_buffer"], opt2.state[q]["momentum_buffer"])
    assert opt2.param_groups[0]["weight_decay"] == 1e-4 and opt2.failed() == []


@pytest.mark.parametrize("n,p", [(3, 1), (16, 16), (33, 7), (64, 64)])
def test_reference_step_stays_on_the_manifold(n, p):
    rng = np.random.default_rng(n * 100 + p)
    x = R.qr_pos(rng.standard_normal((n, p)))
    g, m = rng.standard_normal((n, p)), rng.standard_normal((n, p))
    for mom, nest in ((0.0, False), (0.9, False), (0.9, True)):
        xn, mn = R.step(x, g, m, 0.01, mom, 0.0, 0.05, nest)
        assert R.orth_error(xn) <= 1e-14
        if mom > 0:
            assert np.abs(R.sym(xn.T @ mn)).max() <= 1e-13 * max(1.0, np.abs(mn).max())   # transported: tangent at X+
        else:
            assert np.array_equal(mn, m)
    # the retraction is the unique QR factor with a positive diagonal
    y = rng.standard_normal((n, p))
    q = R.qr_pos(y)
    assert np.all(np.diag(q.T @ y) > 0) and np.abs(np.tril(q.T @ y, -1)).max() <= 1e-12


def test_failure_flags_of_replaced_plans_are_still_reported():
    from tadmm import riemannian, stf_layers
    m = stf_layers.StfTKConv2dC(12, 16, 3, hp_dict=HP, name="k")
    opt = riemannian.StiefelSGD(m.named_parameters(), lr=0.1)
    assert opt.failed() == []
    opt._old_flags[id(m.last_kernel)] = torch.ones(1, dtype=torch.int32)       # what a plan rebuild keeps of the old plan
    opt._old_flags[id(m.first_kernel)] = torch.zeros(1, dtype=torch.int32)
    assert opt.failed() == ["last_kernel"]
