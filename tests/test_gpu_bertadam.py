"""The native BertAdam step (csrc/bertadam.hip, `ops.BertAdamPlan`, `tadmm.optimization.BertAdam`) on the device.

Shapes come from K = ops.BERTADAM_CHUNK: tensors of 1, 3, 4, 5, 255, 256, 257, K-1, K, K+1, 2K+3 and 3K+5 elements in ONE
plan (single chunks, whole chunks, several chunks with a short last one, tails of 1 .. 3 elements).  The 3K+5 tensor and
the 5-element one are views at a 4-byte offset in all four arrays; the K+1 tensor has only p off the 16-byte grid (the norm
launch reads it 16 bytes at a time, the update launch by elements).  Tensors alternate between a gradient norm far above
max_grad_norm and far below it, so every plan mixes clipped and unclipped tensors.

The reference is `ops.bert_adam_composed` in float64 on the same float32 inputs; the metric is max|a - ref| / max|ref| and
the bar the project's 1e-5 (the reference optimiser's own float32 run stays within 3.1e-7 of its float64 run on p, m and v
over five steps at such sizes).  Measured on an MI355X over all sixteen (case, steps) pairs, worst of p, m, v:
    weight_decay 0 and 0.01 alike (decay adds one rounding to p only):
    max_grad_norm 1,  (b1, b2) = (0.9, 0.999):  1 step 1.02e-7,  3 steps 2.56e-7
    max_grad_norm 1,  (b1, b2) = (0.5, 0.9):    1 step 1.65e-7,  3 steps 2.90e-7
    max_grad_norm -1, (b1, b2) = (0.9, 0.999):  1 step 1.17e-7,  3 steps 2.28e-7
    max_grad_norm -1, (b1, b2) = (0.5, 0.9):    1 step 1.08e-7,  3 steps 1.96e-7
    grad_norms() against float64 numpy: 1.7e-16 relative;  the optimiser on the five fixture cases: 3.2e-7 at worst
Gradient norms (double accumulation of at most 3K+5 terms, bound near n 2^-53) are held to 1e-11 relative against numpy.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import _bertadam_ref as R
from _unaligned import guards_intact, misaligned
from tadmm import _cabi, ops
from tadmm.optimization import BertAdam

pytestmark = pytest.mark.gpu

K = ops.BERTADAM_CHUNK
NUMELS = [1, 3, 4, 5, 255, 256, 257, K - 1, K, K + 1, 2 * K + 3, 3 * K + 5]
ALL_OFF = {3 * K + 5: (1, 2, 3, 1), 5: (3, 1, 1, 2)}       # 4-byte offsets of p, g, m, v
P_OFF = {K + 1: (1, 0, 0, 0)}
STEPS = 3
LR, EPS = 1e-2, 1e-6
INVALID = -1                                               # TADMM_ERR_INVALID


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def inputs():
    """Host float32 inputs, made once: p, m, v (a state a few steps into training) and STEPS gradients per tensor."""
    g = torch.Generator().manual_seed(1717)
    data = []
    for j, n in enumerate(NUMELS):
        p = torch.randn(n, generator=g)
        m = 0.1 * torch.randn(n, generator=g)
        v = 0.01 * torch.rand(n, generator=g)
        scale = 30.0 if j % 2 == 0 else 1e-3 / n ** 0.5     # norm far above 1 / far below 1
        grads = [scale * torch.randn(n, generator=g) for _ in range(STEPS)]
        data.append((p, m, v, grads))
    return data


def _place(t, off, dev):
    t = t.to(dev)
    return misaligned(t, off) if off else t.clone()


def _device_set(inputs, dev, grads_at=0):
    out = []
    for (p, m, v, grads), n in zip(inputs, NUMELS):
        offs = ALL_OFF.get(n) or P_OFF.get(n) or (0, 0, 0, 0)
        out.append(tuple(_place(t, o, dev) for t, o in zip((p, grads[grads_at], m, v), offs)))
    return out


_REF = {}


def _reference(inputs, wd, mgn, betas, lr=LR):
    """p, m, v in float64 after each of STEPS composed steps; computed once per case and kept unchanged."""
    key = (wd, mgn, betas, lr)
    if key not in _REF:
        ps = [p.double() for p, _, _, _ in inputs]
        ms = [m.double() for _, m, _, _ in inputs]
        vs = [v.double() for _, _, v, _ in inputs]
        snaps = []
        for k in range(STEPS):
            ops.bert_adam_composed(ps, [gr[k].double() for _, _, _, gr in inputs], ms, vs, lr, betas[0], betas[1], EPS,
                                   wd, mgn)
            snaps.append(tuple([t.numpy().copy() for t in ts] for ts in (ps, ms, vs)))
        _REF[key] = snaps
    return _REF[key]


def _worst(tensors, snap):
    worst = 0.0
    for j, (p, _, m, v) in enumerate(tensors):
        for got, ref in ((p, snap[0][j]), (m, snap[1][j]), (v, snap[2][j])):
            worst = max(worst, R.rel_err(got.cpu().numpy(), ref))
    return worst


def _run(tensors, inputs, steps, lr, betas, wd, mgn, plan=None):
    plan = plan or ops.BertAdamPlan(tensors)
    for k in range(steps):
        if k:
            for (_, g, _, _), (_, _, _, grads) in zip(tensors, inputs):
                g.copy_(grads[k])
        plan.step(lr, betas[0], betas[1], EPS, wd, mgn)
    return plan


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)])
@pytest.mark.parametrize("mgn", [1.0, -1])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_agrees_with_composed_float64(dev, inputs, wd, mgn, betas):
    ref = _reference(inputs, wd, mgn, betas)
    tensors = _device_set(inputs, dev)
    plan = _run(tensors, inputs, 1, LR, betas, wd, mgn)
    one = _worst(tensors, ref[0])
    for k in range(1, STEPS):
        for (_, g, _, _), (_, _, _, grads) in zip(tensors, inputs):
            g.copy_(grads[k])
        plan.step(LR, betas[0], betas[1], EPS, wd, mgn)
    three = _worst(tensors, ref[STEPS - 1])
    print(f"bertadam wd={wd} max_grad_norm={mgn} betas={betas}: 1 step {one:.3e}, {STEPS} steps {three:.3e}")
    assert one <= R.BAR and three <= R.BAR
    for t in tensors:
        for x in t:
            assert x._base is None or guards_intact(x)


def test_grad_norms_and_untouched_gradients(dev, inputs):
    tensors = _device_set(inputs, dev)
    before = [g.clone() for _, g, _, _ in tensors]
    plan = ops.BertAdamPlan(tensors)
    assert float(plan.grad_norms().abs().max()) == 0.0
    plan.step(LR, 0.9, 0.999, EPS, 0.01, 1.0)
    norms = plan.grad_norms()
    assert norms.dtype == torch.float64 and norms.device == dev and norms.shape == (len(NUMELS),)
    want = np.array([np.sqrt((gr[0].numpy().astype(np.float64) ** 2).sum()) for _, _, _, gr in inputs])
    err = np.abs(norms.cpu().numpy() - want) / want
    print("bertadam grad_norms: worst relative error", err.max())
    assert err.max() <= 1e-11
    assert (want[0::2] > 2).all() and (want[1::2] < 0.01).all()          # clipped and unclipped in one plan
    for (_, g, _, _), b in zip(tensors, before):                         # g is read only
        assert torch.equal(g, b)
    plan.step(LR, 0.9, 0.999, EPS, 0.01, -1)                             # an unclipped step leaves the norms
    assert np.array_equal(plan.grad_norms().cpu().numpy(), norms.cpu().numpy())


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_zero_gradient_only_decays(dev, inputs, wd):
    tensors = [(p, torch.zeros_like(g), torch.zeros_like(m), torch.zeros_like(v))
               for p, g, m, v in _device_set(inputs, dev)]
    start = [p.clone() for p, _, _, _ in tensors]
    ops.BertAdamPlan(tensors).step(LR, 0.9, 0.999, EPS, wd, 1.0)
    for (p, _, m, v), p0 in zip(tensors, start):
        assert not m.any() and not v.any()
        if wd == 0:
            assert torch.equal(p, p0)
        else:       # c = 1, u = wd p: p - lr (wd p), three float32 roundings; one ulp of slack
            want = p0 - (p0 * wd) * LR
            assert R.rel_err(p.cpu().numpy(), want.cpu().numpy()) <= 2.0 ** -23


def test_zero_rate_keeps_p_and_advances_moments(dev, inputs):
    ref = _reference(inputs, 0.01, 1.0, (0.9, 0.999), lr=0.0)
    tensors = _device_set(inputs, dev)
    start = [p.clone() for p, _, _, _ in tensors]
    ops.BertAdamPlan(tensors).step(0.0, 0.9, 0.999, EPS, 0.01, 1.0)
    for j, ((p, _, m, v), p0) in enumerate(zip(tensors, start)):
        assert torch.equal(p, p0)
        assert not torch.equal(m, inputs[j][1].to(dev)) and not torch.equal(v, inputs[j][2].to(dev))
        assert R.rel_err(m.cpu().numpy(), ref[0][1][j]) <= R.BAR and R.rel_err(v.cpu().numpy(), ref[0][2][j]) <= R.BAR


def test_bitwise_repeatable(dev, inputs):
    runs = []
    for _ in range(2):
        tensors = _device_set(inputs, dev)
        plan = _run(tensors, inputs, STEPS, LR, (0.9, 0.999), 0.01, 1.0)
        runs.append(([t.clone() for ts in tensors for t in ts], plan.grad_norms().clone()))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][1], runs[1][1])


# ---------------------------------------------------------------------- optimiser level
@pytest.mark.parametrize("case", ["main", "beyond", "noclip", "nosched", "inf"])
def test_optimizer_reproduces_fixture(dev, case):
    """`inf`: the same elements are NaN as in the reference's run, all others finite (`check_step`)."""
    index, arr = R.fixture()
    params = R.make_params(index, arr, dev)
    opt = R.make_optimizer(BertAdam, index, params, index["cases"][case]["hyper"])
    worst = 0.0
    for k in range(index["steps"]):
        R.set_grads(index, arr, params, k, case)
        opt.step()
        worst = max(worst, R.check_step(index, arr, opt, params, case, k))
        np.testing.assert_allclose(opt.get_lr(), index["cases"][case]["get_lr"][k + 1], rtol=1e-15, atol=0)
    print(f"bertadam optimiser, fixture case {case}: worst {worst:.3e}")
    assert [len(opt._plans[gi]) for gi in range(len(index["groups"]))] == [1, 1]       # one plan per group


def test_late_gradient_gets_its_own_plan_and_counter(dev):
    index, arr = R.fixture()
    hyper = index["cases"]["main"]["hyper"]
    sets = [R.make_params(index, arr, d) for d in (dev, torch.device("cpu"))]
    opts = [R.make_optimizer(BertAdam, index, ps, hyper) for ps in sets]
    for k in range(4):
        for ps, opt in zip(sets, opts):
            R.set_grads(index, arr, ps, k, "main")
            if k < 2:
                ps[0].grad = None                     # tensor 0 of group 0 gains a gradient at step 2
            opt.step()
    opt, ps = opts[0], sets[0]
    assert [opt.state[p]["step"] for p in ps] == [2, 4, 4, 4, 4]
    assert len(opt._plans[0]) == 2 and len(opt._plans[1]) == 1
    for a, b in zip(sets[0], sets[1]):                # against the composed route, which the CPU tests hold to the fixture
        for x, y in ((a, b), (opts[0].state[a]["next_m"], opts[1].state[b]["next_m"]),
                     (opts[0].state[a]["next_v"], opts[1].state[b]["next_v"])):
            assert R.rel_err(x.detach().cpu().numpy(), y.detach().numpy()) <= R.BAR


def test_gradients_zeroed_in_place_are_not_staged(dev):
    index, arr = R.fixture()
    params = R.make_params(index, arr, dev)
    opt = R.make_optimizer(BertAdam, index, params, index["cases"]["nosched"]["hyper"])
    weights = [torch.from_numpy(arr[f"grad_1_{i}"].copy()).to(dev) for i in range(len(params))]
    R.set_grads(index, arr, params, 0, "nosched")
    opt.step()
    ptrs = [p.grad.data_ptr() for p in params]
    plans = [ent[1] for gi in opt._plans for ent in opt._plans[gi].values()]
    opt.zero_grad(set_to_none=False)
    sum((p * w).sum() for p, w in zip(params, weights)).backward()
    opt.step()
    assert [p.grad.data_ptr() for p in params] == ptrs
    assert [ent[1] for gi in opt._plans for ent in opt._plans[gi].values()] == plans
    for i, p in enumerate(params):                    # and the step used what accumulated there
        assert torch.equal(p.grad, weights[i])
        assert R.rel_err(p.detach().cpu().numpy(), arr[f"nosched_p_1_{i}"]) <= R.BAR


def test_state_dict_round_trip_continues_identically(dev):
    index, arr = R.fixture()
    hyper = index["cases"]["main"]["hyper"]
    a = R.make_params(index, arr, dev)
    opt_a = R.make_optimizer(BertAdam, index, a, hyper)
    for k in range(2):
        R.set_grads(index, arr, a, k, "main")
        opt_a.step()
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    opt_b = R.make_optimizer(BertAdam, index, b, dict(lr=1.0, schedule="none"))
    opt_b.load_state_dict(copy.deepcopy(opt_a.state_dict()))
    for k in range(2, 4):
        for ps, opt in ((a, opt_a), (b, opt_b)):
            R.set_grads(index, arr, ps, k, "main")
            opt.step()
    for x, y in zip(a, b):
        assert opt_a.state[x]["step"] == opt_b.state[y]["step"] == 4
        assert torch.equal(x, y) and torch.equal(opt_a.state[x]["next_m"], opt_b.state[y]["next_m"])
        assert torch.equal(opt_a.state[x]["next_v"], opt_b.state[y]["next_v"])


def test_bfloat16_parameters_take_the_composed_route(dev):
    index, arr = R.fixture()
    hyper = index["cases"]["nosched"]["hyper"]
    params = R.make_params(index, arr, dev, dtype=torch.bfloat16)
    opt = R.make_optimizer(BertAdam, index, params, hyper)
    twin = [p.detach().clone() for p in params]
    ms, vs = [torch.zeros_like(t) for t in twin], [torch.zeros_like(t) for t in twin]
    for k in range(2):
        R.set_grads(index, arr, params, k, "nosched")
        opt.step()
        for g in index["groups"]:
            ops.bert_adam_composed([twin[i] for i in g["params"]], [params[i].grad for i in g["params"]],
                                   [ms[i] for i in g["params"]], [vs[i] for i in g["params"]], hyper["lr"], hyper["b1"],
                                   hyper["b2"], hyper["e"], g["weight_decay"], hyper["max_grad_norm"])
    assert not any(opt._plans.get(gi) for gi in range(len(index["groups"])))
    for i, p in enumerate(params):
        assert p.dtype == torch.bfloat16 and opt.state[p]["next_m"].dtype == torch.bfloat16
        assert torch.equal(p.detach(), twin[i]) and torch.equal(opt.state[p]["next_m"], ms[i])
        assert torch.equal(opt.state[p]["next_v"], vs[i])
    with pytest.raises(_cabi.TadmmError):
        ops.BertAdamPlan([(twin[0], twin[0].clone(), ms[0], vs[0])])


# ---------------------------------------------------------------------- ABI refusals
def test_abi_refusals_launch_nothing(dev):
    h = ops._handle(dev)
    lib = h.lib
    p, g, m, v = (torch.full((8,), x, device=dev) for x in (1.0, 2.0, 3.0, 4.0))

    def desc(p=p, g=g, m=m, v=v, n=8, shift=(0, 0, 0, 0)):
        d = _cabi.BertAdamDesc()
        d.p, d.g, d.m, d.v = (None if t is None else t.data_ptr() + s for t, s in zip((p, g, m, v), shift))
        d.n = n
        return (_cabi.BertAdamDesc * 1)(d)

    size = C.c_size_t()
    assert lib.tadmm_bertadam_workspace_bytes(1, desc(), C.byref(size)) == 0 and size.value > 0
    ws = torch.empty(size.value, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    bad = [(0, desc()), (-1, desc()), (1, desc(p=None)), (1, desc(g=None)), (1, desc(m=None)), (1, desc(v=None)),
           (1, desc(shift=(2, 0, 0, 0))), (1, desc(shift=(0, 1, 0, 0))), (1, desc(shift=(0, 0, 0, 3))),
           (1, desc(n=0)), (1, desc(n=-5))]
    for n, arr in bad:
        plan = C.c_void_p()
        assert lib.tadmm_bertadam_workspace_bytes(n, arr, C.byref(size)) == INVALID
        assert lib.tadmm_bertadam_plan_create(h.ptr, n, arr, ws.data_ptr(), ws.numel(), stream, C.byref(plan)) == INVALID
        assert not plan.value
    assert lib.tadmm_bertadam_workspace_bytes(1, None, C.byref(size)) == INVALID
    plan = ops.BertAdamPlan([(p, g, m, v)])
    for args in [(1e-3, 1.0, 0.999, 1e-6), (1e-3, -0.1, 0.999, 1e-6), (1e-3, 0.9, 1.0, 1e-6), (1e-3, 0.9, -1.0, 1e-6),
                 (1e-3, 0.9, 0.999, -1e-6), (-1e-3, 0.9, 0.999, 1e-6), (float("nan"), 0.9, 0.999, 1e-6)]:
        assert lib.tadmm_bertadam_step(plan._plan, *args, 0.01, 1.0, stream) == INVALID
        with pytest.raises(_cabi.TadmmError):
            plan.step(*args, 0.01, 1.0)
    assert lib.tadmm_bertadam_step(None, 1e-3, 0.9, 0.999, 1e-6, 0.01, 1.0, stream) == INVALID
    torch.cuda.synchronize(dev)
    for t, x in ((p, 1.0), (g, 2.0), (m, 3.0), (v, 4.0)):
        assert bool((t == x).all())
    assert float(plan.grad_norms()[0]) == 0.0                            # no norm launch ran either
    plan.step(1e-3, 0.9, 0.999, 1e-6, 0.01, 1.0)                         # the same plan still works
    assert abs(float(plan.grad_norms()[0]) - 32.0 ** 0.5) <= 1e-12
