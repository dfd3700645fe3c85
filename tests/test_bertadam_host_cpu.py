"""BertAdam on the CPU (the composed route, `ops.bert_adam_composed`) and the schedules against the G17 fixture, which
was recorded from the reference's own optimiser in float32.  The bar on p, next_m and next_v is the project's 1e-5 on
max|a - ref| / max|ref| (both sides are float32 runs of the same arithmetic; they differ by the rounding of a few
operations).  Schedule multipliers are host doubles and agree to 1e-15."""
import importlib
import logging
import os
import sys

import numpy as np
import pytest
import torch

import _bertadam_ref as R
from tadmm import ops, optimization
from tadmm.optimization import BertAdam

CPU = torch.device("cpu")


@pytest.mark.parametrize("case", ["main", "beyond", "noclip", "nosched", "inf"])
def test_composed_route_reproduces_fixture(case):
    index, arr = R.fixture()
    hyper = index["cases"][case]["hyper"]
    params = R.make_params(index, arr, CPU)
    opt = R.make_optimizer(BertAdam, index, params, hyper)
    lrs = index["cases"][case]["get_lr"]
    assert opt.get_lr() == [0] == lrs[0]
    for k in range(index["steps"]):
        R.set_grads(index, arr, params, k, case)
        before = [p.grad.clone() for p in params]
        opt.step()
        R.check_step(index, arr, opt, params, case, k)
        np.testing.assert_allclose(opt.get_lr(), lrs[k + 1], rtol=1e-15, atol=0)
        for p, g in zip(params, before):                     # gradients are not written back
            assert torch.equal(torch.nan_to_num(p.grad), torch.nan_to_num(g))


def test_first_step_under_warmup_moves_nothing_but_updates_moments():
    index, arr = R.fixture()
    params = R.make_params(index, arr, CPU)
    opt = R.make_optimizer(BertAdam, index, params, index["cases"]["main"]["hyper"])
    R.set_grads(index, arr, params, 0, "main")
    opt.step()
    for i, p in enumerate(params):
        assert np.array_equal(p.detach().numpy(), arr[f"init_{i}"])
        assert opt.state[p]["next_m"].abs().max() > 0 and opt.state[p]["next_v"].abs().max() > 0


def test_schedule_multipliers():
    index, _ = R.fixture()
    assert {str(k): v.__name__ for k, v in optimization.SCHEDULES.items()} == index["schedules"]
    seen = set()
    for g in index["schedule_grid"]:
        s = getattr(optimization, g["class"])(t_total=g["t_total"], **g["kwargs"])
        assert isinstance(s, optimization._LRSchedule)
        got = [s.get_lr(k, nowarn=True) for k in range(len(g["mult"]))]
        assert np.abs(np.array(got) - np.array(g["mult"])).max() <= 1e-15, g["class"]
        seen.add(g["class"])
    assert seen == {"ConstantLR", "WarmupConstantSchedule", "WarmupLinearSchedule", "WarmupCosineSchedule",
                    "WarmupCosineWithHardRestartsSchedule", "WarmupCosineWithWarmupRestartsSchedule"}
    assert optimization.WarmupLinearSchedule(warmup=0.1, t_total=-1).get_lr(7) == 1.0     # no t_total: no schedule


def test_schedule_validation_and_warning(caplog):
    with pytest.raises(ValueError, match=r"Invalid warmup: 1.0 - should be in \[0.0, 1.0\[ or -1"):
        optimization.WarmupLinearSchedule(warmup=1.0, t_total=10)
    with pytest.raises(AssertionError):
        optimization.WarmupCosineWithHardRestartsSchedule(warmup=0.1, t_total=10, cycles=0.5)
    with pytest.raises(AssertionError):
        optimization.WarmupCosineWithWarmupRestartsSchedule(warmup=0.5, t_total=10, cycles=2.0)
    s = optimization.WarmupLinearSchedule(warmup=0.1, t_total=10)
    with caplog.at_level(logging.WARNING, logger=optimization.logger.name):
        assert s.get_lr(10) == 0.0 and not caplog.records             # progress == 1: still inside
        assert s.get_lr(12) == 0.0
        assert len(caplog.records) == 1 and "Training beyond specified 't_total'" in caplog.records[0].getMessage()
        assert "WarmupLinearSchedule" in caplog.records[0].getMessage()
        s.get_lr(12)                                                  # the same progress again: no second warning
        s.get_lr(11)
        assert len(caplog.records) == 1
        s.get_lr(13, nowarn=True)
        assert len(caplog.records) == 1
        optimization.WarmupConstantSchedule(warmup=0.1, t_total=10).get_lr(50)    # a schedule without the warning
        assert len(caplog.records) == 1
        optimization.ConstantLR(t_total=-1)
        assert "t_total value of -1 results in schedule not being applied" in caplog.records[-1].getMessage()


@pytest.mark.parametrize("kwargs, message", [
    (dict(lr=-1.0), "Invalid learning rate: -1.0 - should be >= 0.0"),
    (dict(lr=1e-3, schedule="cosine"), "Invalid schedule parameter: cosine"),
    (dict(lr=1e-3, b1=1.0), r"Invalid b1 parameter: 1.0 - should be in \[0.0, 1.0\["),
    (dict(lr=1e-3, b1=-0.1), r"Invalid b1 parameter: -0.1 - should be in \[0.0, 1.0\["),
    (dict(lr=1e-3, b2=1.5), r"Invalid b2 parameter: 1.5 - should be in \[0.0, 1.0\["),
    (dict(lr=1e-3, e=-1e-6), "Invalid epsilon value: -1e-06 - should be >= 0.0"),
    (dict(lr=1e-3, warmup=1.5, t_total=10), r"Invalid warmup: 1.5 - should be in \[0.0, 1.0\[ or -1"),
])
def test_constructor_validation(kwargs, message):
    with pytest.raises(ValueError, match=message):
        BertAdam([torch.nn.Parameter(torch.zeros(3))], **kwargs)


def test_constructor_defaults_and_schedule_object(caplog):
    p = torch.nn.Parameter(torch.zeros(3))
    opt = BertAdam([p], lr=1e-3)
    g = opt.param_groups[0]
    assert (g["b1"], g["b2"], g["e"], g["weight_decay"], g["max_grad_norm"]) == (0.9, 0.999, 1e-6, 0.01, 1.0)
    assert type(g["schedule"]) is optimization.WarmupLinearSchedule and g["schedule"].t_total == -1.0
    own = optimization.WarmupCosineSchedule(warmup=0.1, t_total=20)
    with caplog.at_level(logging.WARNING, logger=optimization.logger.name):
        opt = BertAdam([p], lr=1e-3, schedule=own, warmup=0.2)
    assert opt.param_groups[0]["schedule"] is own
    assert any("ineffective when _LRSchedule object is provided" in r.getMessage() for r in caplog.records)
    with pytest.raises(ValueError):                      # torch's own refusal of a missing lr
        BertAdam([p])


def _saved_state(index, arr):
    sd = index["state_dict"]
    groups = []
    for g in sd["param_groups"]:
        g = dict(g)
        s = g["schedule"]
        g["schedule"] = getattr(optimization, s["class"])(warmup=s["warmup"], t_total=s["t_total"])
        groups.append(g)
    state = {int(i): {"step": sd["step"][str(i)], "next_m": torch.from_numpy(arr[f"sd_m_{i}"].copy()),
                      "next_v": torch.from_numpy(arr[f"sd_v_{i}"].copy())} for i in sd["state_keys"]}
    return {"state": state, "param_groups": groups}


def test_reference_state_loads_and_training_continues():
    index, arr = R.fixture()
    after = index["state_after"]
    params = R.make_params(index, arr, CPU, source="main_p_%d_{i}" % (after - 1))
    # built with other hyper-parameters: the loaded param groups carry the recorded ones
    opt = R.make_optimizer(BertAdam, index, params, dict(lr=1.0, schedule="none", max_grad_norm=-1))
    opt.load_state_dict(_saved_state(index, arr))
    np.testing.assert_allclose(opt.get_lr(), index["cases"]["main"]["get_lr"][after], rtol=1e-15)
    for k in range(after, index["steps"]):
        R.set_grads(index, arr, params, k, "main")
        opt.step()
        R.check_step(index, arr, opt, params, "main", k)


def test_state_dict_has_the_reference_layout():
    index, arr = R.fixture()
    params = R.make_params(index, arr, CPU)
    opt = R.make_optimizer(BertAdam, index, params, index["cases"]["main"]["hyper"])
    for k in range(index["state_after"]):
        R.set_grads(index, arr, params, k, "main")
        opt.step()
    sd, want = opt.state_dict(), index["state_dict"]
    assert sorted(sd["state"]) == want["state_keys"]
    for i, s in sd["state"].items():
        assert sorted(s) == want["entry_keys"] and type(s["step"]) is int and s["step"] == want["step"][str(i)]
        assert R.rel_err(s["next_m"].numpy(), arr[f"sd_m_{i}"]) <= R.BAR
        assert R.rel_err(s["next_v"].numpy(), arr[f"sd_v_{i}"]) <= R.BAR
    for g, w in zip(sd["param_groups"], want["param_groups"]):
        assert set(g) == set(w)
        assert {k: v for k, v in g.items() if k != "schedule"} == {k: v for k, v in w.items() if k != "schedule"}
        assert type(g["schedule"]).__name__ == w["schedule"]["class"]
        assert (g["schedule"].warmup, g["schedule"].t_total) == (w["schedule"]["warmup"], w["schedule"]["t_total"])


def test_parameter_without_gradient_is_left_alone():
    index, arr = R.fixture()
    params = R.make_params(index, arr, CPU)
    opt = R.make_optimizer(BertAdam, index, params, index["cases"]["nosched"]["hyper"])
    R.set_grads(index, arr, params, 0, "nosched")
    params[1].grad = None
    opt.step()
    assert len(opt.state[params[1]]) == 0 and opt.get_lr() == [0]
    assert np.array_equal(params[1].detach().numpy(), arr["init_1"])
    R.set_grads(index, arr, params, 1, "nosched")
    opt.step()                                               # two classes now: counters 1 and 0
    assert [opt.state[p]["step"] for p in params] == [2, 1, 2, 2, 2]
    held = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state[params[1]].items()}
    value = params[1].detach().clone()
    R.set_grads(index, arr, params, 2, "nosched")
    params[1].grad = None
    opt.step()
    assert [opt.state[p]["step"] for p in params] == [3, 1, 3, 3, 3]
    assert torch.equal(params[1].detach(), value)
    assert torch.equal(opt.state[params[1]]["next_m"], held["next_m"])
    assert torch.equal(opt.state[params[1]]["next_v"], held["next_v"])
    # the others went on exactly as in the recorded run
    for i in (0, 2, 3, 4):
        assert R.rel_err(params[i].detach().numpy(), arr[f"nosched_p_2_{i}"]) <= R.BAR


def test_sparse_gradients_raise():
    p = torch.nn.Parameter(torch.zeros(4, 3))
    opt = BertAdam([p], lr=1e-3)
    p.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 3))
    with pytest.raises(RuntimeError, match="Adam does not support sparse gradients, please consider SparseAdam instead"):
        opt.step()
    with pytest.raises(RuntimeError, match="sparse gradients"):
        ops.bert_adam_composed([p.detach()], [p.grad], [torch.zeros(4, 3)], [torch.zeros(4, 3)], 1e-3)


def test_composed_route_in_float64_and_on_strided_tensors():
    g = torch.Generator().manual_seed(5)
    base = torch.randn(6, 8, generator=g, dtype=torch.float64)
    p, p2 = base.clone().t(), base.clone().t().contiguous()          # a non-contiguous view and its dense copy
    grad = torch.randn(8, 6, generator=g, dtype=torch.float64)
    st = [torch.zeros(8, 6, dtype=torch.float64) for _ in range(4)]
    n1 = ops.bert_adam_composed([p], [grad], [st[0]], [st[1]], 1e-2, 0.9, 0.999, 1e-6, 0.01, 1.0)
    n2 = ops.bert_adam_composed([p2], [grad], [st[2]], [st[3]], 1e-2, 0.9, 0.999, 1e-6, 0.01, 1.0)
    assert torch.equal(p, p2) and torch.equal(st[0], st[2]) and torch.equal(st[1], st[3])
    assert abs(float(n1[0]) - float(grad.norm())) <= 1e-12 * float(grad.norm()) and torch.equal(n1[0], n2[0])
    # the rule itself, written out
    c = min(1.0, 1.0 / (float(grad.norm()) + 1e-6))
    m = 0.1 * c * grad
    v = 0.001 * (c * grad) ** 2
    want = base.t() - 1e-2 * (m / (v.sqrt() + 1e-6) + 0.01 * base.t())
    assert (p - want).abs().max() <= 1e-14 * want.abs().max()
    assert ops.bert_adam_composed([], [], [], [], 1e-3) is None
    assert not ops.bert_adam_native(p2, grad, st[2], st[3])          # CPU float64: never the kernel's


def test_module_is_exported_and_dropin_alias_imports():
    import tadmm
    assert tadmm.optimization is optimization and tadmm.BertAdam is BertAdam
    assert ops.BERTADAM_CHUNK % 4 == 0 and ops.BERTADAM_CHUNK >= 256
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dropin = os.path.join(here, "dnn-compression-tensor-admm_amd", "dropin")
    spec = importlib.util.spec_from_file_location("dropin_optimization", os.path.join(dropin, "optimization.py"))
    mod = importlib.util.module_from_spec(spec)
    path = list(sys.path)
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.path[:] = path
    assert mod.BertAdam is BertAdam and mod.SCHEDULES is optimization.SCHEDULES
    assert mod.WarmupLinearSchedule is optimization.WarmupLinearSchedule
