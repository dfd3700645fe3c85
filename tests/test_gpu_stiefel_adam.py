"""GPU checks of Riemannian Adam on Stiefel factors (csrc/stiefel.hip `stiefel_adam_kernel`, tadmm.ops.StiefelPlan.adam_step,
tadmm.riemannian.StiefelAdam) against the float64 restatement of tests/_stiefel_adam_ref.py.

Shapes: those of tests/test_gpu_stiefel.py -- one column, a square factor, sizes that are no multiple of the 4 x 4
register tile or of 16, the largest factor of stftkc_resnet32 (64 x 64), a strided view (ld = p + 3) and one factor just
beyond the LDS bound (124 x 64), which takes the composed device route.  Errors are max |a - ref| / max |ref| against
float64 and the bar is the project's 1e-5: the float32 Householder restatement of one and of five dependent steps stays
within 6.4e-7 of float64 on X, M and v at all these shapes, so the bar applies as it is.  The tests print their figures;
the table is in DESIGN.md section 15.

Measured on an MI355X:
  item 1 (one step, 8 shapes x 12 runs): X+ <= 6.5e-8, M+ <= 8.3e-8, v+ and vmax+ <= 4.2e-8
  item 2 (three steps from zero state): worst 1.2e-7
  item 4 (second pass, pivot spread 6.8e4 .. 8.2e4, cond(Y) 261 .. 286): X+ <= 2.5e-6, M+ <= 2.4e-6; the float32 restatement
         with LAPACK's single-precision QR is at 5.0e-6 .. 1.3e-5 on X+ and 2.0e-6 .. 2.1e-5 on M+
  item 5 (200 steps): max|X^T X - I| 3.0e-8 .. 7.4e-8 on the device, 4.5e-7 .. 8.7e-7 for float32 Householder on the CPU
  item 9 (five optimiser steps): worst one-step error 8.5e-8
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _stiefel_adam_ref as A

pytestmark = pytest.mark.gpu

BAR = 1e-5                                                   # the project's fp32 parity bar
SHAPES = [(3, 1), (16, 16), (24, 20), (33, 7), (64, 23), (64, 64)]
CASES = [(n, p, 0) for n, p in SHAPES] + [(24, 20, 3), (124, 64, 0)]        # (n, p, ld - p)
IDS = [f"{n}x{p}" + (f"+ld{e}" if e else "") for n, p, e in CASES]
TWO_PASS_STEP = [(33, 7, 0), (64, 32, 0), (40, 20, 3), (64, 23, 3)]
GRID = [(ams, wd, betas) for ams in (False, True) for wd in (0.0, 0.05) for betas in ((0.9, 0.999), (0.5, 0.9))]


def _dev():
    return torch.device("cuda", 0)


def _put(a: np.ndarray, extra: int) -> torch.Tensor:
    """float32 device copy of a; with `extra` > 0 a view of a wider buffer (row stride p + extra) filled with a marker."""
    n, p = a.shape
    buf = torch.full((n, p + extra), 7.0, dtype=torch.float32, device=_dev())
    v = buf[:, :p] if extra else buf
    v.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
    return v


def _inputs(n, p, seed):
    """X orthonormal, a Gaussian G and a Gaussian projected onto the tangent space at X as exp_avg; float32 arrays."""
    rng = np.random.default_rng(seed)
    x = A.qr_pos(rng.standard_normal((n, p))).astype(np.float32)
    g = rng.standard_normal((n, p)).astype(np.float32)
    m = A.tangent(x, rng.standard_normal((n, p))).astype(np.float32)
    return x, g, m


def _rel(a, ref) -> float:
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max()
    return float(np.abs(a - ref).max() / scale) if scale > 0 else float(np.abs(a).max())


def _state(plan, v, vmax, t):
    """Per-factor lists -> the three state tensors of `adam_step`, in the plan's slot order."""
    o = plan.order
    return (torch.tensor([v[i] for i in o], dtype=torch.float32, device=_dev()),
            torch.tensor([vmax[i] for i in o], dtype=torch.float32, device=_dev()),
            torch.tensor([t[i] for i in o], dtype=torch.int32, device=_dev()))


def _of(plan, tensor, i):
    return tensor[plan.slot_of(i)].item()


def test_cases_are_on_both_sides_of_the_resident_bound():
    from tadmm import ops
    assert all(ops.stiefel_fits(n, p) for n, p, _ in CASES[:-1]) and not ops.stiefel_fits(*CASES[-1][:2])
    assert all(ops.stiefel_fits(n, p) for n, p, _ in TWO_PASS_STEP)


# ---------------------------------------------------------------------------------------------------- item 1
@pytest.mark.parametrize("n,p,extra", CASES, ids=IDS)
def test_one_step_from_a_nontrivial_state(n, p, extra):
    from tadmm import ops
    x, g, m = _inputs(n, p, 1000 + n * 7 + p)
    s0 = float((A.tangent(x, g) ** 2).sum())
    v0 = float(np.float32(0.5 * s0))                       # v' lies between v0 and ~s0
    lr, eps = 0.05, 1e-8
    worst = dict(x=0.0, m=0.0, v=0.0, vmax=0.0)
    for ams, wd, betas in GRID:
        for vm0 in ((float(np.float32(4.0 * s0)), float(np.float32(0.25 * v0))) if ams else (0.0,)):
            X, G, M = _put(x, extra), _put(g, extra), _put(m, extra)
            plan = ops.StiefelPlan([(X, G, M)])
            assert (len(plan.native), len(plan.composed)) == ((1, 0) if ops.stiefel_fits(n, p) else (0, 1))
            V, VM, T = _state(plan, [v0], [vm0], [3])
            plan.adam_step(lr, betas, eps, wd, ams, V, VM, T)
            xr, mr, vr, vmr, tr = A.step(x, g, m, v0, vm0, 3, lr, betas, eps, wd, ams)
            if ams:
                assert (vm0 > vr) == (vm0 > v0)            # the two cases: vmax above and below v'
            err = dict(x=_rel(X, xr), m=_rel(M, mr), v=_rel(V, [vr]), vmax=_rel(VM, [vmr]))
            for k, e in err.items():
                worst[k] = max(worst[k], e)
                assert e <= BAR, (ams, wd, betas, vm0, k, e)
            if not ams:
                assert VM.item() == 0.0                    # not touched without amsgrad
            assert T.item() == 4 and tr == 4
            assert plan.failed() == []
            if extra:                                      # nothing written between the rows
                assert bool((X._base[:, p:] == 7.0).all()) and bool((M._base[:, p:] == 7.0).all())
    print(f"stiefel adam step {n}x{p} ld+{extra}: max rel err X+ {worst['x']:.3e}  M+ {worst['m']:.3e}  "
          f"v+ {worst['v']:.3e}  vmax+ {worst['vmax']:.3e}  (bar {BAR:.0e})")


# ---------------------------------------------------------------------------------------------------- item 2
def test_three_steps_from_zero_state():
    """Bias corrections at t = 1, 2, 3 and a transported exp_avg feeding the next step.  The composed factor comes FIRST
    in the plan, so the state arrays' slot order differs from the factor order."""
    from tadmm import ops
    cases = [CASES[-1]] + CASES[:-1]
    lr, wd, betas = 0.05, 0.05, (0.9, 0.999)
    for ams in (False, True):
        rng = np.random.default_rng(77)
        xs = [_inputs(n, p, 400 + i)[0] for i, (n, p, _) in enumerate(cases)]
        grads = [[rng.standard_normal((n, p)).astype(np.float32) for _ in range(3)] for n, p, _ in cases]
        X = [_put(x, e) for x, (_, _, e) in zip(xs, cases)]
        G = [_put(np.zeros((n, p)), e) for n, p, e in cases]
        M = [_put(np.zeros((n, p)), e) for n, p, e in cases]
        plan = ops.StiefelPlan(list(zip(X, G, M)))
        assert plan.order == list(range(1, len(cases))) + [0]
        zero = [0.0] * len(cases)
        V, VM, T = _state(plan, zero, zero, [0] * len(cases))
        ref = [(x.astype(np.float64), np.zeros(x.shape), 0.0, 0.0, 0) for x in xs]
        worst = 0.0
        for k in range(3):
            for Gd, gs in zip(G, grads):
                Gd.copy_(torch.from_numpy(gs[k]))
            plan.adam_step(lr, betas, 1e-8, wd, ams, V, VM, T)
            ref = [A.step(r[0], gs[k], r[1], r[2], r[3], r[4], lr, betas, 1e-8, wd, ams) for r, gs in zip(ref, grads)]
            for i, ((n, p, e), r) in enumerate(zip(cases, ref)):
                errs = (_rel(X[i], r[0]), _rel(M[i], r[1]), _rel([_of(plan, V, i)], [r[2]]))
                if ams:
                    errs += (_rel([_of(plan, VM, i)], [r[3]]),)
                worst = max(worst, *errs)
                assert max(errs) <= BAR, (ams, k, n, p, e, errs)
                assert _of(plan, T, i) == k + 1
        assert plan.failed() == []
        print(f"stiefel adam, three steps from zero state (amsgrad {ams}): worst rel err {worst:.3e}  (bar {BAR:.0e})")


# ---------------------------------------------------------------------------------------------------- item 3
def test_zero_gradient_from_zero_state():
    from tadmm import ops
    xs = [_inputs(n, p, 500 + i)[0] for i, (n, p, _) in enumerate(CASES)]
    X = [_put(x, e) for x, (_, _, e) in zip(xs, CASES)]
    G = [_put(np.zeros((n, p)), e) for n, p, e in CASES]
    M = [_put(np.zeros((n, p)), e) for n, p, e in CASES]
    plan = ops.StiefelPlan(list(zip(X, G, M)))
    zero = [0.0] * len(CASES)
    V, VM, T = _state(plan, zero, zero, [0] * len(CASES))
    plan.adam_step(0.05, (0.9, 0.999), 1e-8, 0.0, False, V, VM, T)
    assert plan.failed() == []
    for i, x in enumerate(xs):
        xr, mr, vr, _, tr = A.step(x, np.zeros_like(x), np.zeros_like(x), 0.0, 0.0, 0, 0.05)
        assert _rel(X[i], xr) <= BAR and bool(torch.isfinite(X[i]).all()) and bool(torch.isfinite(M[i]).all())
        assert float(M[i].abs().max()) <= BAR * 1.0 and vr == 0.0 and tr == 1
    assert bool((V == 0).all()) and T.cpu().tolist() == [1] * len(CASES)


# ------------------------------------------------------------------------------- item 4: the second Cholesky-QR pass
def _pivot_spread(y: np.ndarray) -> float:
    """max / min squared Cholesky pivot of Y^T Y in float64: what the kernel compares with its second-pass threshold."""
    y = np.asarray(y, dtype=np.float64)
    d = np.diag(np.linalg.cholesky(y.T @ y)) ** 2
    return float(d.max() / d.min())


def test_step_with_a_two_pass_retraction():
    """From zero state the direction has unit Frobenius length whatever the gradient's size, so a gradient in column 0
    alone with lr = 300 stretches that column of Y by ~300: a pivot spread of ~9e4, beyond the second-pass threshold."""
    from tadmm import ops
    lr = 300.0
    for i, (n, p, e) in enumerate(TWO_PASS_STEP):
        x = _inputs(n, p, 800 + i)[0]
        g = np.zeros((n, p), dtype=np.float32)
        g[:, 0] = np.random.default_rng(850 + i).standard_normal(n).astype(np.float32)
        z = np.zeros((n, p), dtype=np.float32)
        y = A.pre_retraction(x, g, z, 0.0, 0.0, 0, lr)[0]
        spread, cond = _pivot_spread(y), float(np.linalg.cond(y))
        assert spread > ops.STIEFEL_SECOND_PASS, (n, p, spread)            # checked on the CPU: the second pass is taken
        X, G, M = _put(x, e), _put(g, e), _put(z, e)
        plan = ops.StiefelPlan([(X, G, M)])
        assert len(plan.native) == 1
        V, VM, T = _state(plan, [0.0], [0.0], [0])
        plan.adam_step(lr, (0.9, 0.999), 1e-8, 0.0, False, V, VM, T)
        xr, mr, vr, _, _ = A.step(x, g, z, 0.0, 0.0, 0, lr)
        x32, m32, _, _, _ = A.step_f32(x, g, z, 0.0, 0.0, 0, lr)
        ex, em, ev = _rel(X, xr), _rel(M, mr), _rel(V, [vr])
        print(f"stiefel adam step, two passes {n}x{p} ld+{e}: pivot spread {spread:.2e}  cond {cond:.0f}  max rel err "
              f"X+ {ex:.3e}  M+ {em:.3e}  v+ {ev:.3e}   float32 Householder on the CPU: X+ {_rel(x32, xr):.3e}  "
              f"M+ {_rel(m32, mr):.3e}")
        assert plan.failed() == [] and T.item() == 1
        assert ex <= BAR and em <= BAR and ev <= BAR, (n, p, ex, em, ev)
        if e:
            assert bool((X._base[:, p:] == 7.0).all()) and bool((M._base[:, p:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------- item 5
def test_200_steps_stay_on_the_manifold():
    from tadmm import ops
    steps, lr = 200, 0.05
    gen = torch.Generator().manual_seed(3)
    xs = [_inputs(n, p, 50 + i)[0] for i, (n, p, _) in enumerate(CASES)]
    grads = [torch.randn(steps, n, p, generator=gen) / float(np.sqrt(n * p)) for n, p, _ in CASES]   # ||G||_F ~ 1
    want = []                                                              # the yardstick: float32 Householder on the CPU
    for x, gs in zip(xs, grads):
        st, worst = (x, np.zeros_like(x), 0.0, 0.0, 0), 0.0
        gs = gs.numpy()
        for k in range(steps):
            st = A.step_f32(st[0], gs[k], st[1], st[2], st[3], st[4], lr)
            worst = max(worst, A.orth_error(st[0]))
        want.append(worst)
    X = [_put(x, e) for x, (_, _, e) in zip(xs, CASES)]
    G = [_put(np.zeros((n, p)), e) for n, p, e in CASES]
    M = [_put(np.zeros((n, p)), e) for n, p, e in CASES]
    gdev = [g.to(_dev()) for g in grads]
    plan = ops.StiefelPlan(list(zip(X, G, M)))
    zero = [0.0] * len(CASES)
    V, VM, T = _state(plan, zero, zero, [0] * len(CASES))
    eyes = [torch.eye(p, dtype=torch.float64, device=_dev()) for _, p, _ in CASES]
    worst = [torch.zeros((), dtype=torch.float64, device=_dev()) for _ in CASES]
    for k in range(steps):
        torch._foreach_copy_(G, [g[k] for g in gdev])
        plan.adam_step(lr, (0.9, 0.999), 1e-8, 0.0, False, V, VM, T)
        for i, x in enumerate(X):
            xd = x.double()
            worst[i] = torch.maximum(worst[i], (xd.t() @ xd - eyes[i]).abs().max())
    assert plan.failed() == []
    assert T.cpu().tolist() == [steps] * len(CASES) and bool(torch.isfinite(V).all()) and bool((V > 0).all())
    for (n, p, e), x, m, got, ref in zip(CASES, X, M, worst, want):
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(m).all())
        got = float(got)
        print(f"stiefel adam drift {n}x{p} ld+{e}: max over {steps} steps of max|X^T X - I|: device {got:.3e}  "
              f"float32 Householder on the CPU {ref:.3e}")
        assert got <= 4.0 * ref, (n, p, e, got, ref)


# ---------------------------------------------------------------------------------------------------- item 6
def test_grouping_and_repeatability_are_bitwise():
    from tadmm import ops
    data = [_inputs(n, p, 200 + i) for i, (n, p, _) in enumerate(CASES)]
    v0 = [0.3 + 0.1 * i for i in range(len(CASES))]
    vm0 = [0.1 if i % 2 else 50.0 for i in range(len(CASES))]
    t0 = [i for i in range(len(CASES))]

    def run(grouped):
        fac = [tuple(_put(a, e) for a in d) for d, (_, _, e) in zip(data, CASES)]
        out = []
        if grouped:
            plan = ops.StiefelPlan(fac)
            V, VM, T = _state(plan, v0, vm0, t0)
            plan.adam_step(0.01, (0.9, 0.999), 1e-8, 0.05, True, V, VM, T)
            sc = [(_of(plan, V, i), _of(plan, VM, i), _of(plan, T, i)) for i in range(len(fac))]
        else:
            sc = []
            for i, f in enumerate(fac):
                plan = ops.StiefelPlan([f])
                V, VM, T = _state(plan, [v0[i]], [vm0[i]], [t0[i]])
                plan.adam_step(0.01, (0.9, 0.999), 1e-8, 0.05, True, V, VM, T)
                sc.append((V.item(), VM.item(), T.item()))
        for (x, _, m), s in zip(fac, sc):
            out.append((x.cpu().clone(), m.cpu().clone(), s))
        return out

    a, b, c = run(True), run(False), run(True)
    for i, ((xa, ma, sa), (xb, mb, sb), (xc, mc, sc)) in enumerate(zip(a, b, c)):
        assert torch.equal(xa, xb) and torch.equal(ma, mb) and sa == sb, i        # one plan per factor
        assert torch.equal(xa, xc) and torch.equal(ma, mc) and sa == sc, i        # the same step twice
        assert sa[2] == t0[i] + 1


# ---------------------------------------------------------------------------------------------------- item 7
def test_skipped_factor_keeps_everything():
    from tadmm import ops
    data = [_inputs(n, p, 300 + i) for i, (n, p, _) in enumerate(CASES)]
    fac = [tuple(_put(a, e) for a in d) for d, (_, _, e) in zip(data, CASES)]
    skip = (2, len(CASES) - 1)                                          # a resident factor and the composed one
    plan = ops.StiefelPlan([(x, None if i in skip else g, m) for i, (x, g, m) in enumerate(fac)])
    v0 = [float(np.float32(0.4 + 0.1 * i)) for i in range(len(CASES))]
    vm0 = [float(np.float32(0.2 + 0.3 * i)) for i in range(len(CASES))]
    V, VM, T = _state(plan, v0, vm0, [5] * len(CASES))
    plan.adam_step(0.01, (0.9, 0.999), 1e-8, 0.0, True, V, VM, T)
    for i, ((x0, g0, m0), (x, _, m)) in enumerate(zip(data, fac)):
        if i in skip:
            assert torch.equal(x.cpu(), torch.from_numpy(x0)) and torch.equal(m.cpu(), torch.from_numpy(m0))
            assert (_of(plan, V, i), _of(plan, VM, i), _of(plan, T, i)) == (v0[i], vm0[i], 5)
        else:
            xr, mr, vr, vmr, _ = A.step(x0, g0, m0, v0[i], vm0[i], 5, 0.01, amsgrad=True)
            assert _rel(x, xr) <= BAR and _rel(m, mr) <= BAR
            assert _rel([_of(plan, V, i)], [vr]) <= BAR and _rel([_of(plan, VM, i)], [vmr]) <= BAR
            assert _of(plan, T, i) == 6
    assert plan.failed() == []


# ---------------------------------------------------------------------------------------------------- item 8
def test_nan_gradient_fails_one_factor_and_writes_nothing_of_it():
    from tadmm import ops
    idx = (1, 5, len(CASES) - 1)                           # 16 x 16, 64 x 64 (resident) and 124 x 64 (composed)
    for bad in (1, len(CASES) - 1):                        # the failing factor: on the native route, on the composed one
        data = [_inputs(*CASES[i][:2], 600 + i) for i in idx]
        data[idx.index(bad)][1][2, 0] = np.nan
        fac = [tuple(_put(a, 0) for a in d) for d in data]
        plan = ops.StiefelPlan(fac)
        v0, vm0 = [0.5, 0.75, 1.25], [0.25, 2.5, 0.125]
        V, VM, T = _state(plan, v0, vm0, [3, 4, 5])
        plan.adam_step(0.01, (0.9, 0.999), 1e-8, 0.0, True, V, VM, T)
        torch.cuda.synchronize()                           # the launch finished normally
        assert plan.failed() == [idx.index(bad)]
        for k, ((x0, g0, m0), (x, _, m)) in enumerate(zip(data, fac)):
            if idx[k] == bad:
                assert torch.equal(x.cpu(), torch.from_numpy(x0)) and torch.equal(m.cpu(), torch.from_numpy(m0))
                assert (_of(plan, V, k), _of(plan, VM, k), _of(plan, T, k)) == (v0[k], vm0[k], 3 + k)
            else:
                xr, mr, vr, vmr, _ = A.step(x0, g0, m0, v0[k], vm0[k], 3 + k, 0.01, amsgrad=True)
                assert _rel(x, xr) <= BAR and _rel(m, mr) <= BAR
                assert _rel([_of(plan, V, k)], [vr]) <= BAR and _rel([_of(plan, VM, k)], [vmr]) <= BAR
                assert _of(plan, T, k) == 4 + k


# ---------------------------------------------------------------------------------------------------- item 9
class _HP:
    ranks = {"a": [8, 8], "b": [8, 8]}


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from tadmm import stf_layers
        self.c1 = stf_layers.StfTKConv2dC(16, 16, 3, padding=1, hp_dict=_HP, name="a")
        self.c2 = stf_layers.StfTKConv2dC(16, 16, 3, padding=1, hp_dict=_HP, name="b")
        self.head = torch.nn.Linear(16, 10)

    def forward(self, x):
        return self.head(self.c2(torch.relu(self.c1(x))).mean((2, 3)))


_STF = ("c1.first_kernel", "c1.last_kernel", "c2.first_kernel", "c2.last_kernel")


def _np(t):
    return t.detach().cpu().double().numpy()


@pytest.mark.parametrize("amsgrad", [False, True], ids=["adam", "amsgrad"])
def test_end_to_end_training(amsgrad):
    from tadmm import riemannian
    dev, steps, lr, wd = _dev(), 5, 0.01, 0.0
    torch.manual_seed(33)
    net = _Net().to(dev)
    g = torch.Generator().manual_seed(34)
    x, t = torch.randn(4, 16, 8, 8, generator=g).to(dev), torch.randn(4, 10, generator=g).to(dev)
    net.eval()                                             # no mode switch from here on: only the optimiser's writes
    with torch.no_grad():                                  # can invalidate the inference caches this forward fills
        y_start = net(x)
    opt = riemannian.StiefelAdam(net.named_parameters(), lr=lr, amsgrad=amsgrad, stabilize=10)
    assert len(opt.stiefel_params()) == 4 and len(opt.state) == 0
    named = dict(net.named_parameters())
    euclid = [k for k in named if k not in _STF]
    twin = {k: torch.nn.Parameter(named[k].detach().clone()) for k in euclid}
    twin_opt = torch.optim.Adam(list(twin.values()), lr=lr, amsgrad=amsgrad)
    losses, worst = [], 0.0
    for k in range(steps):
        loss = F.mse_loss(net(x), t)
        losses.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        before = {}
        for name in _STF:                                  # (b) the state each factor's step starts from
            p, st = named[name], opt.state.get(named[name], {})
            assert (len(st) == 0) == (k == 0)
            before[name] = (_np(p), _np(p.grad), _np(st["exp_avg"]) if st else np.zeros(p.shape),
                            float(st["exp_avg_sq"].item()) if st else 0.0,
                            float(st["max_exp_avg_sq"].item()) if st and amsgrad else 0.0,
                            int(st["step"].item()) if st else 0)
        for name in euclid:
            twin[name].grad = named[name].grad.detach().clone()
        opt.step()
        twin_opt.step()
        for name in euclid:                                # (a) torch's Adam on the same gradients, bit for bit
            assert torch.equal(named[name].detach(), twin[name].detach()), (k, name)
        for name in _STF:
            p, st = named[name], opt.state[named[name]]
            x0, g0, m0, v0, vm0, t0 = before[name]
            xr, mr, vr, vmr, tr = A.step(x0, g0, m0, v0, vm0, t0, lr, (0.9, 0.999), 1e-8, wd, amsgrad)
            assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].numel() == 1 and st["step"].numel() == 1
            assert st["exp_avg_sq"].is_cuda and st["step"].is_cuda and ("max_exp_avg_sq" in st) == amsgrad
            errs = [_rel(p, xr), _rel(st["exp_avg"], mr), _rel(st["exp_avg_sq"], [vr])]
            if amsgrad:
                errs.append(_rel(st["max_exp_avg_sq"], [vmr]))
            worst = max(worst, *errs)
            assert max(errs) <= BAR, (k, name, errs)
            assert int(st["step"].item()) == tr == k + 1
    assert opt.failed() == []                              # (c)
    with torch.no_grad():
        y_end = net(x)
        print(f"stiefel adam end to end (amsgrad {amsgrad}): loss {losses[0]:.6f} -> {float(F.mse_loss(y_end, t)):.6f}; "
              f"worst one-step rel err of X+, exp_avg, exp_avg_sq over {steps} steps: {worst:.3e}  (bar {BAR:.0e})")
        fresh = _Net().to(dev)                             # (d) no stale inference cache
        fresh.load_state_dict(net.state_dict())
        fresh.eval()
        assert torch.equal(y_end, fresh(x)) and not torch.equal(y_end, y_start)
    # (e) the optimiser's state round-trips and the next step is the same bit for bit
    sd = copy.deepcopy(opt.state_dict())                   # as a checkpoint would: state_dict() hands out the live buffers
    clone = _Net().to(dev)
    clone.load_state_dict(net.state_dict())
    clone.eval()
    opt2 = riemannian.StiefelAdam(clone.named_parameters(), lr=lr, amsgrad=amsgrad)
    opt2.load_state_dict(sd)
    for n_, o_ in ((net, opt), (clone, opt2)):
        l_ = F.mse_loss(n_(x), t)
        o_.zero_grad()
        l_.backward()
        o_.step()
    for (k, a), (_, b) in zip(net.named_parameters(), clone.named_parameters()):
        assert torch.equal(a, b), k
        sa, sb = opt.state[a], opt2.state[b]
        assert set(sa) == set(sb)
        for key in sa:
            assert torch.equal(sa[key].cpu(), sb[key].cpu()), (k, key)
    assert int(opt2.state[dict(clone.named_parameters())[_STF[0]]]["step"].item()) == steps + 1
    assert opt2.failed() == []


# ---------------------------------------------------------------------------------------------------- item 10
def test_the_active_set_changes():
    from tadmm import riemannian, stf_layers
    shapes = [(16, 16), (33, 7), (64, 23)]
    lr, skipper = 0.05, 1
    rng = np.random.default_rng(91)
    xs = [_inputs(n, p, 900 + i)[0] for i, (n, p) in enumerate(shapes)]
    grads = [[rng.standard_normal(s).astype(np.float32) for _ in range(3)] for s in shapes]
    params = [stf_layers.StiefelParameter(torch.from_numpy(x).to(_dev())) for x in xs]
    opt = riemannian.StiefelAdam(params, lr=lr)
    ref = [(x.astype(np.float64), np.zeros(x.shape), 0.0, 0.0, 0) for x in xs]
    for k in range(3):
        kept = None
        for i, p in enumerate(params):
            if k == 1 and i == skipper:
                p.grad = None
                st = opt.state[p]
                kept = (p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), st["step"].clone())
            else:
                p.grad = torch.from_numpy(grads[i][k]).to(_dev())
                ref[i] = A.step(ref[i][0], grads[i][k], ref[i][1], ref[i][2], ref[i][3], ref[i][4], lr)
        opt.step()
        if kept is not None:                               # untouched at the step it sat out
            st = opt.state[params[skipper]]
            assert torch.equal(params[skipper].detach(), kept[0]) and torch.equal(st["exp_avg"], kept[1])
            assert torch.equal(st["exp_avg_sq"], kept[2]) and torch.equal(st["step"], kept[3]) and kept[3].item() == 1
        for i, p in enumerate(params):
            st = opt.state[p]
            assert int(st["step"].item()) == ref[i][4] == (k + 1 if i != skipper or k == 0 else k)
            errs = (_rel(p, ref[i][0]), _rel(st["exp_avg"], ref[i][1]), _rel(st["exp_avg_sq"], [ref[i][2]]))
            assert max(errs) <= BAR, (k, i, errs)
    assert opt.failed() == []
