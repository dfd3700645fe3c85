"""GPU checks of the Riemannian SGD step on the Stiefel manifold (csrc/stiefel.hip, tadmm.ops.StiefelPlan,
tadmm.riemannian.StiefelSGD, tadmm.stf_layers.StfTKConv2dC) against the float64 restatement of tests/_stiefel_ref.py.

Shapes: the smallest at which the kernel can go wrong -- one column, a square factor, sizes that are no multiple of the
4 x 4 register tile or of 16, the largest factor of stftkc_resnet32 (64 x 64), a strided view (ld = p + 3) and one
factor just beyond the LDS bound (124 x 64), which takes the composed device route.

Measured on an MI355X (the tests print their figures; the table is in DESIGN.md section 14):
  case 1 (one step, 8 shapes x 8 hyper-parameter sets): max|X+ - ref| / max|ref| <= 6.5e-8, M+ <= 7.5e-8 (bar 1e-5)
  case 2 (200 steps): max|X^T X - I| 3.9e-8 .. 7.4e-8 on the device, 3.3e-7 .. 9.4e-7 for float32 Householder on the CPU
  case 3 (project): Q within 5.4e-8 of float64, max|Q^T Q - I| <= 7.2e-8 (CPU float32: 1.7e-7 .. 5.5e-7)
  second pass (graded columns, pivot spread 6.6e4 .. 7.9e5; every case above runs one pass): project Q within 4.9e-8,
          step X+ within 9.3e-8 and M+ within 1.6e-7 of float64
  case 7 (five optimiser steps of a two-layer stack): parameter error 1.5e-7 on the device; the float32 CPU
          restatement of the same five steps is at 6.1e-7, within the 1e-5 bar of float64 (checked when the test was
          written, and again by the test), so the bar is 1e-5.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _stiefel_ref as R

pytestmark = pytest.mark.gpu

BAR = 1e-5                                                   # the project's fp32 parity bar
SHAPES = [(3, 1), (16, 16), (24, 20), (33, 7), (64, 23), (64, 64)]
CASES = [(n, p, 0) for n, p in SHAPES] + [(24, 20, 3), (124, 64, 0)]        # (n, p, ld - p)
IDS = [f"{n}x{p}" + (f"+ld{e}" if e else "") for n, p, e in CASES]
HYPER = [(mom, nest, wd) for mom in (0.0, 0.9) for nest in (False, True) for wd in (0.0, 0.05)]
PROJECT_SEED = 11


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
    """X orthonormal (reference QR of a seeded Gaussian, rounded to float32), Gaussian G and M, all float32 arrays."""
    rng = np.random.default_rng(seed)
    x = R.qr_pos(rng.standard_normal((n, p))).astype(np.float32)
    g = rng.standard_normal((n, p)).astype(np.float32)
    m = rng.standard_normal((n, p)).astype(np.float32)
    return x, g, m


def _safe_lr(x, g, m):
    # ||d|| <= 2 ||g|| + ||M|| with ||g|| <= ||G|| + wd ||X||: lr ||d||_F <= 0.5
    return 0.5 / (2.0 * (np.linalg.norm(g) + 0.05 * np.linalg.norm(x)) + np.linalg.norm(m))


def _rel(a: torch.Tensor, ref: np.ndarray) -> float:
    return float(np.abs(a.detach().cpu().double().numpy() - ref).max() / np.abs(ref).max())


def _orth(a: torch.Tensor) -> float:
    return R.orth_error(a.detach().cpu().double().numpy())


def test_cases_are_on_both_sides_of_the_resident_bound():
    from tadmm import ops
    assert all(ops.stiefel_fits(n, p) for n, p, _ in CASES[:-1]) and not ops.stiefel_fits(*CASES[-1][:2])


# ---------------------------------------------------------------------------------------------------- case 1
@pytest.mark.parametrize("n,p,extra", CASES, ids=IDS)
def test_one_step_against_float64(n, p, extra):
    from tadmm import ops
    x, g, m = _inputs(n, p, 1000 + n * 7 + p)
    lr = _safe_lr(x, g, m)
    worst_x = worst_m = 0.0
    for mom, nest, wd in HYPER:
        X, G, M = _put(x, extra), _put(g, extra), _put(m, extra)
        plan = ops.StiefelPlan([(X, G, M)])
        assert (len(plan.native), len(plan.composed)) == ((1, 0) if ops.stiefel_fits(n, p) else (0, 1))
        plan.step(lr, mom, 0.0, wd, nest)
        xr, mr = R.step(x, g, m, lr, mom, 0.0, wd, nest)
        ex = _rel(X, xr)
        worst_x = max(worst_x, ex)
        assert ex <= BAR, (mom, nest, wd, ex)
        if mom > 0:
            em = _rel(M, mr)
            worst_m = max(worst_m, em)
            assert em <= BAR, (mom, nest, wd, em)
        else:
            assert torch.equal(M.cpu(), torch.from_numpy(m))                  # no momentum: the buffer is not touched
        assert plan.failed() == []
        if extra:                                                              # nothing written between the rows
            assert bool((X._base[:, p:] == 7.0).all()) and bool((M._base[:, p:] == 7.0).all())
    print(f"stiefel step {n}x{p} ld+{extra}: max rel err X+ {worst_x:.3e}  M+ {worst_m:.3e}  (bar {BAR:.0e})")


def test_dampening_against_float64():
    from tadmm import ops
    x, g, m = _inputs(33, 7, 5)
    lr = _safe_lr(x, g, m)
    X, G, M = _put(x, 0), _put(g, 0), _put(m, 0)
    ops.StiefelPlan([(X, G, M)]).step(lr, 0.9, 0.3, 0.0, False)
    xr, mr = R.step(x, g, m, lr, 0.9, 0.3, 0.0, False)
    assert _rel(X, xr) <= BAR and _rel(M, mr) <= BAR


# ---------------------------------------------------------------------------------------------------- case 2
def _step_f32_cpu(x, g, m, lr, mom):
    """The same step in float32 on the CPU with Householder torch.linalg.qr: the yardstick of the orthogonality tests."""
    a = x.t() @ g
    r = g - x @ (0.5 * (a + a.t()))
    m = mom * m + r
    q, rr = torch.linalg.qr(x - lr * m)
    s = torch.sign(torch.diagonal(rr))
    s[s == 0] = 1.0
    q = q * s
    b = q.t() @ m
    return q, m - q @ (0.5 * (b + b.t()))


def test_200_steps_stay_on_the_manifold():
    from tadmm import ops
    steps, lr, mom = 200, 0.05, 0.9
    gen = torch.Generator().manual_seed(3)
    xs = [torch.from_numpy(_inputs(n, p, 50 + i)[0]) for i, (n, p, _) in enumerate(CASES)]
    grads = [torch.randn(steps, n, p, generator=gen) / float(np.sqrt(n * p)) for n, p, _ in CASES]   # ||G||_F ~ 1
    # yardstick
    want = []
    for x, gs in zip(xs, grads):
        m, worst = torch.zeros_like(x), 0.0
        for t in range(steps):
            x, m = _step_f32_cpu(x, gs[t], m, lr, mom)
            worst = max(worst, R.orth_error(x.numpy()))
        want.append(worst)
    # device: all factors in one plan, one launch a step (plus the composed factor)
    X = [_put(x.numpy(), e) for x, (_, _, e) in zip(xs, CASES)]
    G = [_put(np.zeros((n, p)), e) for n, p, e in CASES]
    M = [_put(np.zeros((n, p)), e) for n, p, e in CASES]
    gdev = [g.to(_dev()) for g in grads]
    plan = ops.StiefelPlan(list(zip(X, G, M)))
    eyes = [torch.eye(p, dtype=torch.float64, device=_dev()) for _, p, _ in CASES]
    worst = [torch.zeros((), dtype=torch.float64, device=_dev()) for _ in CASES]
    for t in range(steps):
        torch._foreach_copy_(G, [g[t] for g in gdev])
        plan.step(lr, mom)
        for i, x in enumerate(X):
            xd = x.double()
            worst[i] = torch.maximum(worst[i], (xd.t() @ xd - eyes[i]).abs().max())
    assert plan.failed() == []
    for (n, p, e), got, ref in zip(CASES, worst, want):
        got = float(got)
        print(f"stiefel drift {n}x{p} ld+{e}: max over {steps} steps of max|X^T X - I|: device {got:.3e}  "
              f"float32 Householder on the CPU {ref:.3e}")
        assert got <= 4.0 * ref, (n, p, e, got, ref)


# ---------------------------------------------------------------------------------------------------- case 3
def _xavier(n, p, seed):
    t = torch.empty(n, p)
    torch.manual_seed(seed)
    torch.nn.init.xavier_uniform_(t)
    return t


def test_project_mode():
    from tadmm import ops
    ys = [_xavier(n, p, PROJECT_SEED + i) for i, (n, p, _) in enumerate(CASES)]
    for y in ys:
        assert np.linalg.cond(y.double().numpy()) < 1e4          # the float64 reference itself is meaningful
    X = [_put(y.numpy(), e) for y, (_, _, e) in zip(ys, CASES)]
    plan = ops.stiefel_project_(*X)
    assert plan.failed() == [] and len(plan.native) == len(CASES) - 1
    for (n, p, e), y, x in zip(CASES, ys, X):
        qr = R.qr_pos(y.numpy())
        q32, r32 = torch.linalg.qr(y)
        err, got, ref = _rel(x, qr), _orth(x), R.orth_error(q32.numpy())
        print(f"stiefel project {n}x{p} ld+{e}: cond {np.linalg.cond(y.double().numpy()):.1f}  max rel err Q {err:.3e}  "
              f"max|Q^T Q - I| device {got:.3e}  float32 Householder on the CPU {ref:.3e}")
        assert err <= BAR, (n, p, err)
        assert got <= 4.0 * ref, (n, p, got, ref)


# ------------------------------------------------------------------------------- the second Cholesky-QR pass
TWO_PASS = [(24, 20, 0), (33, 7, 0), (64, 32, 0), (24, 20, 3), (64, 23, 3)]       # resident shapes, two of them strided
TWO_PASS_STEP = [(33, 7, 0), (64, 32, 0), (40, 20, 3), (64, 23, 3)]               # n - p large enough for a graded normal part


def _pivot_spread(y: np.ndarray) -> float:
    """max / min squared Cholesky pivot of Y^T Y in float64: what the kernel compares with its second-pass threshold."""
    y = np.asarray(y, dtype=np.float64)
    d = np.diag(np.linalg.cholesky(y.T @ y)) ** 2
    return float(d.max() / d.min())


def _graded(n, p, seed, top=1000.0):
    """A seeded Gaussian whose column scales are graded from 1 to `top`: well conditioned as a matrix problem for
    float64 (cond ~ top), with a pivot spread of ~ top^2."""
    rng = np.random.default_rng(seed)
    scale = np.logspace(0.0, np.log10(top), p) if p > 1 else np.ones(1)
    return (rng.standard_normal((n, p)) * scale[None, :]).astype(np.float32)


def test_project_takes_the_second_pass_on_graded_columns():
    from tadmm import ops
    ys = [_graded(n, p, 700 + i) for i, (n, p, _) in enumerate(TWO_PASS)]
    for y in ys:                                                 # checked on the CPU: the second pass is really taken
        assert _pivot_spread(y) > 3.0 * ops.STIEFEL_SECOND_PASS and np.linalg.cond(y.astype(np.float64)) < 1e4
    X = [_put(y, e) for y, (_, _, e) in zip(ys, TWO_PASS)]
    plan = ops.stiefel_project_(*X)
    assert plan.failed() == [] and len(plan.native) == len(TWO_PASS)
    for (n, p, e), y, x in zip(TWO_PASS, ys, X):
        q32 = torch.linalg.qr(torch.from_numpy(y))[0]
        err, got, ref = _rel(x, R.qr_pos(y)), _orth(x), R.orth_error(q32.numpy())
        print(f"stiefel project, two passes {n}x{p} ld+{e}: pivot spread {_pivot_spread(y):.2e}  cond "
              f"{np.linalg.cond(y.astype(np.float64)):.0f}  max rel err Q {err:.3e}  max|Q^T Q - I| device {got:.3e}  "
              f"float32 Householder on the CPU {ref:.3e}")
        assert err <= BAR, (n, p, err)
        assert got <= 4.0 * ref, (n, p, got, ref)
        if e:
            assert bool((x._base[:, p:] == 7.0).all())


def test_step_with_a_two_pass_retraction_transports_the_momentum():
    """Y^T Y = I + lr^2 d^T d for a tangent d: a gradient in the normal space of X (X^T G = 0, so r = G) with column
    scales graded from 1 to 1000 and lr = 1 push the pivot spread of a STEP beyond the threshold, so the momentum is
    transported from the tile the second pass wrote.  (Y is formed in float32 before it is factored, so a step's error
    grows with cond(Y) * 2^-24; the cases keep cond(Y) below 2000.)"""
    from tadmm import ops
    lr, mom = 1.0, 0.9
    for i, (n, p, e) in enumerate(TWO_PASS_STEP):
        x, _, m = _inputs(n, p, 800 + i)
        a = x.astype(np.float64)
        z = _graded(n, p, 900 + i)
        g = (z - a @ (a.T @ z)).astype(np.float32)
        r = g - a @ R.sym(a.T @ g)
        y = a - lr * (mom * m + r)
        assert _pivot_spread(y) > 3.0 * ops.STIEFEL_SECOND_PASS and np.linalg.cond(y) < 2000, (n, p, _pivot_spread(y))
        X, G, M = _put(x, e), _put(g, e), _put(m, e)
        plan = ops.StiefelPlan([(X, G, M)])
        plan.step(lr, mom)
        xr, mr = R.step(x, g, m, lr, mom)
        ex, em = _rel(X, xr), _rel(M, mr)
        tangent = float(np.abs(R.sym(X.cpu().double().numpy().T @ M.cpu().double().numpy())).max() / np.abs(mr).max())
        print(f"stiefel step, two passes {n}x{p} ld+{e}: pivot spread {_pivot_spread(y):.2e}  max rel err X+ {ex:.3e}  "
              f"M+ {em:.3e}  sym(X+^T M+) / max|M+| {tangent:.3e}")
        assert plan.failed() == [] and ex <= BAR and em <= BAR, (n, p, ex, em)
        assert tangent <= BAR
        assert _orth(X) <= 4.0 * R.orth_error(torch.linalg.qr(torch.from_numpy(y.astype(np.float32)))[0].numpy())


# ---------------------------------------------------------------------------------------------------- case 4
def test_grouping_and_repeatability_are_bitwise():
    from tadmm import ops
    data = [_inputs(n, p, 200 + i) for i, (n, p, _) in enumerate(CASES)]

    def run(grouped):
        fac = [tuple(_put(a, e) for a in d) for d, (_, _, e) in zip(data, CASES)]
        if grouped:
            ops.StiefelPlan(fac).step(0.01, 0.9, 0.0, 0.05, True)
        else:
            for f in fac:
                ops.StiefelPlan([f]).step(0.01, 0.9, 0.0, 0.05, True)
        return [(x.cpu().clone(), m.cpu().clone()) for x, _, m in fac]

    a, b, c = run(True), run(False), run(True)
    for (xa, ma), (xb, mb), (xc, mc) in zip(a, b, c):
        assert torch.equal(xa, xb) and torch.equal(ma, mb)            # one plan per factor
        assert torch.equal(xa, xc) and torch.equal(ma, mc)            # the same step twice


# ---------------------------------------------------------------------------------------------------- case 5
def test_skipped_factor_keeps_x_and_m():
    from tadmm import ops
    data = [_inputs(n, p, 300 + i) for i, (n, p, _) in enumerate(CASES)]
    fac = [tuple(_put(a, e) for a in d) for d, (_, _, e) in zip(data, CASES)]
    skip = (2, len(CASES) - 1)                                          # a resident factor and the composed one
    plan = ops.StiefelPlan([(x, None if i in skip else g, m) for i, (x, g, m) in enumerate(fac)])
    plan.step(0.01, 0.9, 0.0, 0.0, False)
    for i, ((x0, g0, m0), (x, _, m)) in enumerate(zip(data, fac)):
        if i in skip:
            assert torch.equal(x.cpu(), torch.from_numpy(x0)) and torch.equal(m.cpu(), torch.from_numpy(m0))
        else:
            xr, mr = R.step(x0, g0, m0, 0.01, 0.9)
            assert _rel(x, xr) <= BAR and _rel(m, mr) <= BAR
    assert plan.failed() == []


def test_rank_deficient_projection_sets_the_flag_and_writes_nothing():
    from tadmm import ops
    ys = [_xavier(n, p, PROJECT_SEED + i).numpy().copy() for i, (n, p, _) in enumerate(CASES)]
    bad = (1, 4, len(CASES) - 1)                                        # two resident factors and the composed one
    for i in bad:
        ys[i][:, CASES[i][1] // 2] = 0.0                                # an exactly zero column
    X = [_put(y, e) for y, (_, _, e) in zip(ys, CASES)]
    plan = ops.stiefel_project_(*X)
    torch.cuda.synchronize()                                            # the launch finished normally
    assert plan.failed() == sorted(bad)
    for i, (y, x) in enumerate(zip(ys, X)):
        assert bool(torch.isfinite(x).all())
        if i in bad:
            assert torch.equal(x.cpu(), torch.from_numpy(y))
        else:
            assert _rel(x, R.qr_pos(y)) <= BAR
    # the flag is sticky, and a non-finite gradient is refused the same way in a step
    x, g, m = _inputs(16, 16, 9)
    g[3, 5] = np.inf
    Xs, Gs, Ms = _put(x, 0), _put(g, 0), _put(m, 0)
    p2 = ops.StiefelPlan([(Xs, Gs, Ms)])
    p2.step(0.01, 0.9)
    assert p2.failed() == [0] and torch.equal(Xs.cpu(), torch.from_numpy(x)) and torch.equal(Ms.cpu(), torch.from_numpy(m))
    Gs.copy_(torch.from_numpy(_inputs(16, 16, 9)[1]))
    p2.step(0.01, 0.9)
    assert p2.failed() == [0] and not torch.equal(Xs.cpu(), torch.from_numpy(x))     # sticky flag, healthy step


# ---------------------------------------------------------------------------------------------------- case 6
class _HP:
    ranks = {"a": [8, 8], "b": [8, 8]}


def test_layer_parity_with_tkconv2dc():
    from tadmm import stf_layers, tk_layers
    dev = _dev()
    g = torch.Generator().manual_seed(21)
    W = (torch.randn(16, 16, 3, 3, generator=g) * 0.2).to(dev)
    b = torch.randn(16, generator=g).to(dev)
    stf = stf_layers.StfTKConv2dC(16, 16, 3, padding=1, hp_dict=_HP, name="a", dense_w=W, dense_b=b.clone()).to(dev)
    tk = tk_layers.TKConv2dC(16, 16, 3, padding=1, hp_dict=_HP, name="a", dense_w=W, dense_b=b.clone()).to(dev)
    assert stf.first_kernel.shape == (16, 8) and isinstance(stf.first_kernel, stf_layers.StiefelParameter)
    assert torch.equal(stf.first_kernel.detach().t(), tk.first_kernel.detach()[:, :, 0, 0])
    assert torch.equal(stf.last_kernel.detach(), tk.last_kernel.detach()[:, :, 0, 0])
    assert _orth(stf.first_kernel) <= 1e-5 and _orth(stf.last_kernel) <= 1e-5      # the HOOI factors are on the manifold
    x = torch.randn(2, 16, 8, 8, generator=g).to(dev)
    with torch.no_grad():
        for xx in (x, x.bfloat16()):
            assert torch.equal(stf(xx), tk(xx))
            assert torch.equal(stf.forward_features(xx)[0], tk.forward_features(xx)[0])       # the staged route
    xs, xt = x.clone().requires_grad_(), x.clone().requires_grad_()
    gy = torch.randn(2, 16, 8, 8, generator=g).to(dev)
    ys, yt = stf(xs), tk(xt)
    assert torch.equal(ys, yt)
    ys.backward(gy)
    yt.backward(gy)
    assert torch.equal(xs.grad, xt.grad) and torch.equal(stf.core_kernel.grad, tk.core_kernel.grad)
    assert torch.equal(stf.bias.grad, tk.bias.grad)
    assert torch.equal(stf.first_kernel.grad, tk.first_kernel.grad[:, :, 0, 0].t())
    assert torch.equal(stf.last_kernel.grad, tk.last_kernel.grad[:, :, 0, 0])


# ---------------------------------------------------------------------------------------------------- case 7
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


def _restated_run(params, x, t, steps, lr, mom, dtype):
    """The same training steps restated with library calls in `dtype` on the CPU: F.conv2d, autograd, the Stiefel update
    by tests/_stiefel_ref.py (float64) or float32 Householder QR (float32), torch's SGD rule for the other parameters.
    Returns (final parameters, losses)."""
    P = {k: v.detach().cpu().to(dtype).clone().requires_grad_() for k, v in params.items()}
    x, t = x.cpu().to(dtype), t.cpu().to(dtype)
    buf, losses = {}, []
    for step in range(steps):
        h = x
        for c in ("c1", "c2"):
            h = F.conv2d(h, P[c + ".first_kernel"].t()[:, :, None, None])
            h = F.conv2d(h, P[c + ".core_kernel"], None, 1, 1)
            h = F.conv2d(h, P[c + ".last_kernel"][:, :, None, None], P[c + ".bias"])
            if c == "c1":
                h = torch.relu(h)
        out = F.linear(h.mean((2, 3)), P["head.weight"], P["head.bias"])
        loss = F.mse_loss(out, t)
        losses.append(float(loss.detach()))
        grads = torch.autograd.grad(loss, list(P.values()))
        with torch.no_grad():
            for (k, p), g in zip(P.items(), grads):
                if k in _STF:
                    m = buf.get(k, torch.zeros_like(p))
                    if dtype == torch.float64:
                        xn, mn = R.step(p.numpy(), g.numpy(), m.numpy(), lr, mom)
                        xn, mn = torch.from_numpy(xn), torch.from_numpy(mn)
                    else:
                        xn, mn = _step_f32_cpu(p, g, m, lr, mom)
                    p.copy_(xn)
                    buf[k] = mn
                else:
                    buf[k] = g.clone() if k not in buf else mom * buf[k] + g       # torch.optim.SGD
                    p.sub_(lr * buf[k])
    return {k: v.detach() for k, v in P.items()}, losses


def _max_rel(a, b):
    return max(float((a[k].double() - b[k].double()).abs().max() / b[k].double().abs().max()) for k in b)


def test_end_to_end_training():
    from tadmm import riemannian
    dev, steps, lr, mom = _dev(), 5, 0.05, 0.9
    torch.manual_seed(33)
    net = _Net().to(dev)                                   # built on the CPU, projected onto the manifold by the move
    assert not net.c1._pending_projection
    for k, p in net.named_parameters():
        if k in _STF:
            assert _orth(p) <= 1e-6, k
    g = torch.Generator().manual_seed(34)
    x, t = torch.randn(4, 16, 8, 8, generator=g).to(dev), torch.randn(4, 10, generator=g).to(dev)
    start = {k: p.detach().clone() for k, p in net.named_parameters()}
    ref, ref_losses = _restated_run(start, x, t, steps, lr, mom, torch.float64)
    cpu32, _ = _restated_run(start, x, t, steps, lr, mom, torch.float32)
    cpu_err = _max_rel(cpu32, ref)

    # the whole run stays in eval() mode (the net has no mode-dependent layer): train() / eval() drop the inference
    # caches themselves, so only a run without mode switches shows that the optimiser's writes invalidate them
    net.eval()
    with torch.no_grad():
        y_start = net(x)                                   # fills the inference caches with the initial factors
    opt = riemannian.StiefelSGD(net.named_parameters(), lr=lr, momentum=mom)
    assert len(opt.stiefel_params()) == 4
    losses = []
    for _ in range(steps + 1):
        loss = F.mse_loss(net(x), t)
        losses.append(float(loss.detach()))
        if len(losses) > steps:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    assert opt.failed() == []
    assert losses[steps] < losses[0]
    got = {k: p.detach().cpu() for k, p in net.named_parameters()}
    err = _max_rel(got, ref)
    print(f"stiefel end to end: loss {losses[0]:.6f} -> {losses[steps]:.6f} (float64 {ref_losses[0]:.6f} -> ...); "
          f"max rel parameter error after {steps} steps: device {err:.3e}, float32 CPU restatement {cpu_err:.3e}")
    assert cpu_err <= BAR            # the float32 restatement holds the bar against float64, so the bar applies as it is
    assert err <= BAR, err
    # on the manifold: at most 4x what float32 Householder QR leaves on the same five steps
    for k in _STF:
        assert _orth(got[k]) <= 4.0 * R.orth_error(cpu32[k].numpy()), k
    # no stale plane cache: the eval() forward sees the updated factors, with no mode switch since the caches were filled
    fresh = _Net().to(dev)
    fresh.load_state_dict(net.state_dict())
    fresh.eval()
    with torch.no_grad():
        y0 = net(x)
        assert torch.equal(y0, fresh(x)) and not torch.equal(y0, y_start)
    # and again around one more step: forward, step, forward
    loss = F.mse_loss(net(x), t)
    opt.zero_grad()
    loss.backward()
    with torch.no_grad():
        before = net(x)
    opt.step()
    with torch.no_grad():
        after = net(x)
    fresh.load_state_dict(net.state_dict())
    with torch.no_grad():
        assert torch.equal(after, fresh(x)) and not torch.equal(after, before) and not torch.equal(after, y0)
    # the optimiser's state round-trips and the next step is the same bit for bit
    sd = copy.deepcopy(opt.state_dict())       # as a checkpoint would: state_dict() hands out the live buffers
    twin = _Net().to(dev)
    twin.load_state_dict(net.state_dict())
    opt2 = riemannian.StiefelSGD(twin.named_parameters(), lr=lr, momentum=mom)
    opt2.load_state_dict(sd)
    for n_, o_ in ((net, opt), (twin, opt2)):
        l_ = F.mse_loss(n_(x), t)
        o_.zero_grad()
        l_.backward()
        o_.step()
    for (k, a), (_, b) in zip(net.named_parameters(), twin.named_parameters()):
        assert torch.equal(a, b), k
