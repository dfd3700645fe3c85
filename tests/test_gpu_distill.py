"""Distillation loss on the device (csrc/distill.hip through tadmm.losses / tadmm.functional / tadmm.ops) against the
reference's recorded runs (G15) and the float64 restatement of tests/_distill_ref.py evaluated on the device.

Bars.  With e_f the launch's error and e_c that of `distillation_loss_composed` (torch operations in float32), both
against float64: the loss needs e_f <= 2 max(e_c, 2^-23) (relative); float32 gradients the same in the max norm with the
floor 2^-23 max|g64|; gradients delivered in a 16-bit type are within one unit in the last place of that type at the
reference element's magnitude.  Both sides are float32 row arithmetic of the same length and differ only in summation
order and the exp used, hence the factor two.  Measured on an MI355X: see DESIGN.md section 18.
"""
import pytest
import torch

import _distill_ref as R
from tadmm import functional as HF
from tadmm import losses as L
from tadmm import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2.0 ** -23


def _leaf(x):
    return None if x is None else x.detach().clone().requires_grad_(True)


def _run(fn, s, k, t, target, same=False, gout=None, **kw):
    """(loss, grad_s, grad_k) of one differentiable route; `same`: outputs_kd IS outputs (one gradient, the sum)."""
    base, kd = kw["base"], kw["kd"]
    ls = _leaf(s) if base != "none" else None
    lk = ls if same else (_leaf(k) if kd != "none" else None)
    loss = fn(ls, lk, t if kd != "none" else None, target if base != "none" else None, **kw)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    if gout is None:
        loss.backward()
    else:
        loss.backward(gradient=gout)
    return loss.detach(), None if ls is None else ls.grad, None if (lk is None or same) else lk.grad


def _check_loss(tag, lf, lc, l64):
    """lc None: no composed figure at hand, the floor 2^-23 alone (bar 2^-22).  A reference of exactly zero (one class)
    has no relative error: the errors are absolute there and the floor, a fraction of the reference, is zero."""
    scale = abs(float(l64))
    e_f = abs(float(lf) - float(l64)) / (scale or 1.0)
    e_c = abs(float(lc) - float(l64)) / (scale or 1.0) if lc is not None else 0.0
    print(f"{tag}: loss e_f {e_f:.2e} e_c {e_c:.2e}")
    assert e_f <= 2 * max(e_c, FLOOR if scale else 0.0), (tag, e_f, e_c)
    return e_f, e_c


def _check_grad(tag, what, gf, gc, g64, dtype, scale=1.0):
    """float32: max-norm error against the composed route's (gc None: no composed figure at hand, the floor alone, 2^-22
    max|g64|.  An element is a difference of two probabilities, each within 1.5 units of float32, times a constant; the
    floor holds where the largest element is of the order of the probabilities themselves, as with the random logits of
    scale 3 the callers use); 16-bit: one ulp of the type at every element."""
    g64 = g64 * scale
    assert gf.dtype == dtype and gf.shape == g64.shape
    err = (gf.to(torch.float64) - g64).abs()
    assert bool(torch.isfinite(gf).all()), (tag, what)
    if dtype == torch.float32:
        top = float(g64.abs().max())
        e_f = float(err.max())
        e_c = float((gc.to(torch.float64) - g64).abs().max()) if gc is not None else 0.0
        print(f"{tag}: {what} e_f {e_f / max(top, 1e-300):.2e} e_c {e_c / max(top, 1e-300):.2e} (of max |g|)")
        assert e_f <= 2 * max(e_c, FLOOR * top), (tag, what, e_f, e_c, top)
    else:
        ulps = float((err / R.ulp(g64, dtype)).max())
        print(f"{tag}: {what} worst {ulps:.3f} ulp of {dtype}")
        assert ulps <= 1.0, (tag, what, ulps)


def _compare(tag, s, k, t, target, dtype, same=False, gout=None, scale=1.0, **kw):
    l64, gs64, gk64, _, _ = R.restate(s, k, t, target, **kw)
    if same and gs64 is not None and gk64 is not None:
        gs64, gk64 = gs64 + gk64, None
    lf, gsf, gkf = _run(lambda *a, **q: HF.distillation_loss(*a, route="launch", **q), s, k, t, target, same, gout, **kw)
    lc, gsc, gkc = _run(HF.distillation_loss_composed, s, k, t, target, same, gout, **kw)
    _check_loss(tag, lf, lc, l64)
    if gs64 is not None:
        _check_grad(tag, "grad_s", gsf, gsc, gs64, dtype, scale)
    if gk64 is not None and not same:
        _check_grad(tag, "grad_k", gkf, gkc, gk64, dtype, scale)
    return lf, gsf, gkf


# ------------------------------------------------------------------------------------------------------- G15 parity
def test_module_matches_the_recorded_reference(golden_dir):
    """tadmm.losses.DistillationLoss on the recorded inputs: the reference's float32 CPU loss and gradients.  Bar: both
    are float32 evaluations of one formula; the restatement sits within 1e-6 of the record (test_distill_host_cpu), the
    launch within 2^-22 of the restatement, so 2e-6 relative for the loss and 2e-6 of max|g| for the gradients."""
    for meta in R.golden_index(golden_dir):
        d = {k: v.to(DEV) for k, v in R.recorded(golden_dir, meta["name"]).items()}
        crit = {"ce": torch.nn.CrossEntropyLoss(), "ce_ls": torch.nn.CrossEntropyLoss(label_smoothing=0.1),
                "ce_prob": torch.nn.CrossEntropyLoss()}[meta["criterion"]]
        mod = L.DistillationLoss(crit, lambda inp, t=d["t"]: t, meta["type"], meta["alpha"], meta["tau"])
        s = _leaf(d["s"])
        k = _leaf(d["k"]) if meta["tuple"] else None
        loss = mod(torch.zeros(meta["B"], 1, device=DEV), (s, k) if meta["tuple"] else s, d["target"])
        loss.backward()
        ref = float(d["loss"][0])
        assert abs(float(loss.detach()) - ref) <= 2e-6 * abs(ref), meta
        assert (s.grad - d["grad_s"]).abs().max() <= 2e-6 * d["grad_s"].abs().max(), meta
        if meta["tuple"]:
            got = k.grad if k.grad is not None else torch.zeros_like(k)
            assert (got - d["grad_k"]).abs().max() <= 2e-6 * max(float(d["grad_k"].abs().max()), 1e-30), meta
        assert mod.bad_labels() == 0


# ------------------------------------------------------------------------------------------- case table vs float64
@pytest.mark.parametrize("cid", [c["id"] for c in R.CASES])
def test_case_against_float64(cid):
    case = R.CASE_BY_ID[cid]
    s, k, t, target = R.case_inputs(case, DEV)
    _compare(cid, s, k, t, target, R.DTYPES[case["dtype"]], **R.case_kwargs(case))


def test_scaled_float16_backward():
    """GradScaler's case: the saved gradients are float32 and are multiplied by 2^16 before they are rounded to float16.
    Unscaled, most elements of this gradient are below float16's normal range."""
    s, k, t, target = R.make_inputs(64, 1000, "float16", 77, device=DEV)
    kw = dict(base="index", kd="soft", alpha=0.5, tau=1.0, smoothing=0.0)
    gout = torch.tensor(65536.0, device=DEV)
    _, gs, gk = _compare("scaled-f16", s, k, t, target, torch.float16, gout=gout, scale=65536.0, **kw)
    g64 = R.restate(s, k, t, target, **kw)[2]
    assert float((g64.abs() < 2.0 ** -14).double().mean()) > 0.5        # the premise: unscaled, mostly subnormal


@pytest.mark.parametrize("dtype,peak", [("float32", 1e4), ("float16", 3e4)])
@pytest.mark.parametrize("tau", [1.0, 7.0])
def test_large_logits(dtype, peak, tau):
    s, k, t, target = R.make_inputs(9, 130, "float32", 5, device=DEV)
    dt = R.DTYPES[dtype]
    s, k, t = ((x / x.abs().max() * peak).to(dt) for x in (s, k, t))
    lf, gs, gk = _compare(f"large-{dtype}-tau{tau:g}", s, k, t, target, dt, base="index", kd="soft", alpha=0.5, tau=tau,
                          smoothing=0.1)
    assert bool(torch.isfinite(lf)) and bool(torch.isfinite(gs).all()) and bool(torch.isfinite(gk).all())


def test_teacher_tie_takes_the_first_index():
    s, k, t, target = R.make_inputs(3, 8, "float32", 9, device=DEV)
    t = t.clamp(max=1.0)
    t[:, 2] = 4.0
    t[:, 5] = 4.0
    assert R.teacher_ties(t) == 3
    kw = dict(base="none", kd="hard", alpha=1.0)
    loss, _, gk = _run(lambda *a, **q: HF.distillation_loss(*a, route="launch", **q), s, k, t, target, **kw)
    want = torch.nn.functional.cross_entropy(k.double(), torch.full((3,), 2, device=DEV))
    other = torch.nn.functional.cross_entropy(k.double(), torch.full((3,), 5, device=DEV))
    assert abs(float(want) - float(other)) > 1e-3
    _check_loss("tie", loss, None, want)
    l64, _, gk64, _, _ = R.restate(None, k, t, None, **kw)
    _check_loss("tie", loss, None, l64)
    _check_grad("tie", "grad_k", gk, None, gk64, torch.float32)


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_ignored_and_bad_labels(dtype):
    C = 17
    y = R.label_case(C).to(DEV)
    s, k, t, _ = R.make_inputs(y.numel(), C, dtype, 21, device=DEV)
    crit = L.DistillationLoss(torch.nn.CrossEntropyLoss(label_smoothing=0.1), lambda inp: t, "soft", 0.5, 2.0)
    ls, lk = _leaf(s), _leaf(k)
    loss = crit(None, (ls, lk), y)
    loss.backward()
    l64, gs64, gk64, kept, bad = R.restate(s, k, t, y, base="index", kd="soft", alpha=0.5, tau=2.0, smoothing=0.1)
    assert kept == 4 and bad == 2 and crit.bad_labels() == 2
    # the composed route counts and drops the same rows
    box = []
    kw = dict(base="index", kd="soft", alpha=0.5, tau=2.0, smoothing=0.1)
    lc, gsc, gkc = _run(lambda *a, **q: HF.distillation_loss_composed(*a, counts=box, **q), s, k, t, y, **kw)
    assert box[0].tolist() == [4, 2]
    _check_loss(f"labels-{dtype}", loss.detach(), lc, l64)
    assert float(ls.grad[[1, 3, 4]].abs().max()) == 0.0 and float(ls.grad[[0, 2, 5, 6]].abs().max(dim=1).values.min()) > 0.0
    _check_grad(f"labels-{dtype}", "grad_s", ls.grad, gsc, gs64, R.DTYPES[dtype])
    _check_grad(f"labels-{dtype}", "grad_k", lk.grad, gkc, gk64, R.DTYPES[dtype])
    # nothing kept: NaN, as torch
    allign = torch.full_like(y, -100)
    none = L.DistillationLoss(torch.nn.CrossEntropyLoss(), None, "none", 0.5, 1.0)
    assert bool(torch.isnan(none(None, s, allign))) and none.bad_labels() == 0
    assert bool(torch.isnan(torch.nn.functional.cross_entropy(s.float(), allign)))


@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_row_slices_of_a_stack_and_guards(dtype):
    """outputs = stack[:, 0], outputs_kd = stack[:, 1] of a (B, 2, C) tensor with odd C: the second view starts an odd
    number of elements in, rows are 2C apart; read in place, nothing around them or around the gradients is written."""
    B, C = 6, 131
    dt = R.DTYPES[dtype]
    s, k, t, y = R.make_inputs(B, C, dtype, 31, device=DEV)
    wide = R.misaligned_rows(torch.cat([s, k], dim=1), 0)           # (B, 2C) rows in a guarded buffer
    stack = wide.view(B, 2, C)
    vs, vk = stack[:, 0], stack[:, 1]
    assert vs.stride() == (2 * C, 1) and vk.data_ptr() - vs.data_ptr() == C * s.element_size()
    kw = dict(base="index", kd="soft", alpha=0.5, tau=3.0, smoothing=0.1)
    l64, gs64, gk64, _, _ = R.restate(s, k, t, y, **kw)
    lc, gsc, gkc = _run(HF.distillation_loss_composed, s, k, t, y, **kw)
    gbuf = [R.misaligned_rows(torch.zeros(B, C, device=DEV), off) for off in (4, 12)]
    loss, counts, gs, gk = ops.distill_loss(vs, vk, t, y, out={"grad_s": gbuf[0], "grad_k": gbuf[1]}, **kw)
    assert gs.data_ptr() == gbuf[0].data_ptr() and gk.data_ptr() == gbuf[1].data_ptr()
    _check_loss(f"stack-{dtype}", loss, lc, l64)
    for what, g, gc, g64 in (("grad_s", gs, gsc, gs64), ("grad_k", gk, gkc, gk64)):
        _check_grad(f"stack-{dtype}", what + " (saved float32)", g, gc if dt == torch.float32 else None, g64, torch.float32)
        assert R.guards_intact(g)
    assert R.guards_intact(wide) and torch.equal(vs, s) and torch.equal(vk, k)
    # through autograd: gradients arrive in the views' type and shape
    ls = stack.detach().clone().requires_grad_(True)
    out = HF.distillation_loss(ls[:, 0], ls[:, 1], t, y, route="launch", **kw)
    out.backward()
    assert ls.grad.shape == (B, 2, C) and ls.grad.dtype == dt
    _check_grad(f"stack-{dtype}", "grad_s", ls.grad[:, 0], gsc, gs64, dt)
    _check_grad(f"stack-{dtype}", "grad_k", ls.grad[:, 1], gkc, gk64, dt)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("off", [2, 4, 8])
def test_bases_off_a_16_byte_boundary(dtype, off):
    dt = R.DTYPES[dtype]
    if off % torch.empty(0, dtype=dt).element_size():
        off = 12                               # float32 has no base 2 bytes off: 12 instead
    B, C = 5, 72                               # C a multiple of 8: only the base decides the access width
    s, k, t, y = R.make_inputs(B, C, dtype, 41 + off, device=DEV)
    ms, mk, mt = (R.misaligned_rows(x, off) for x in (s, k, t))
    kw = dict(base="index", kd="soft", alpha=0.5, tau=2.0, smoothing=0.0)
    l64, gs64, gk64, _, _ = R.restate(s, k, t, y, **kw)
    lc, gsc, gkc = _run(HF.distillation_loss_composed, s, k, t, y, **kw)
    loss, _, gs, gk = ops.distill_loss(ms, mk, mt, y, **kw)
    tag = f"off{off}-{dtype}"
    _check_loss(tag, loss, lc, l64)
    for what, g, gc, g64 in (("grad_s", gs, gsc, gs64), ("grad_k", gk, gkc, gk64)):
        _check_grad(tag, what + " (saved float32)", g, gc if dt == torch.float32 else None, g64, torch.float32)
    assert all(R.guards_intact(v) for v in (ms, mk, mt))


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_same_tensor_gets_the_sum(dtype):
    s, _, t, y = R.make_inputs(12, 100, dtype, 51, device=DEV)
    kw = dict(base="index", kd="soft", alpha=0.5, tau=3.0, smoothing=0.0)
    _, g_one, none = _compare(f"same-{dtype}", s, s, t, y, R.DTYPES[dtype], same=True, **kw)
    assert none is None
    # the module with a single tensor does the same
    crit = L.DistillationLoss(torch.nn.CrossEntropyLoss(), lambda inp: t, "soft", 0.5, 3.0)
    ls = _leaf(s)
    crit(None, ls, y).backward()
    assert torch.equal(ls.grad, g_one)


def test_bitwise_reproducible_and_no_host_sync():
    s, k, t, y = R.make_inputs(33, 1000, "float32", 61, device=DEV)
    kw = dict(base="index", kd="soft", alpha=0.5, tau=3.0, smoothing=0.1)
    fn = lambda *a, **q: HF.distillation_loss(*a, route="launch", **q)
    a = _run(fn, s, k, t, y, **kw)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        b = _run(fn, s, k, t, y, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for x, z in zip(a, b):
        assert torch.equal(x, z)
    c = _run(fn, s.half(), k.half(), t.half(), y, base="index", kd="hard", alpha=0.3)
    d = _run(fn, s.half(), k.half(), t.half(), y, base="index", kd="hard", alpha=0.3)
    for x, z in zip(c, d):
        assert torch.equal(x, z)


def _device_kernels(prof):
    from torch.autograd import DeviceType
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    return [n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()]


def test_launch_count():
    """One fused forward is at most two device kernels, one backward at most two."""
    from torch.profiler import ProfilerActivity, profile
    s, k, t, y = R.make_inputs(64, 100, "float16", 71, device=DEV)
    kw = dict(base="index", kd="soft", alpha=0.5, tau=3.0, smoothing=0.1, route="launch")
    ls, lk = _leaf(s), _leaf(k)
    HF.distillation_loss(ls, lk, t, y, **kw).backward()          # warm up: handles, code objects
    probe = torch.ones(8, device=DEV)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as p0:
        probe = probe + 1
        torch.cuda.synchronize()
    assert len(_device_kernels(p0)) == 1, "the profiler does not see device kernels on this machine"
    ls.grad = lk.grad = None
    with profile(activities=[ProfilerActivity.CUDA]) as pf:
        loss = HF.distillation_loss(ls, lk, t, y, **kw)
        torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as pb:
        loss.backward()
        torch.cuda.synchronize()
    fwd, bwd = _device_kernels(pf), _device_kernels(pb)
    print("forward:", fwd, "\nbackward:", bwd)
    assert 1 <= len(fwd) <= 2 and any("distill_rows" in n for n in fwd), fwd
    assert 1 <= len(bwd) <= 2, bwd


@pytest.mark.parametrize("pays", [True, False])
def test_module_follows_the_routing_rule(monkeypatch, pays):
    seen = []
    monkeypatch.setattr(ops, "distill_loss_pays", lambda B, C, dtype, grad=False: seen.append((B, C, dtype, grad)) or pays)
    s, k, t, y = R.make_inputs(16, 100, "float32", 81, device=DEV)
    kw = dict(base="index", kd="hard", alpha=0.5, smoothing=0.1)
    l64, gs64, gk64, _, _ = R.restate(s, k, t, y, **kw)
    crit = L.DistillationLoss(torch.nn.CrossEntropyLoss(label_smoothing=0.1), lambda inp: t, "hard", 0.5, 1.0)
    ls, lk = _leaf(s), _leaf(k)
    loss = crit(None, (ls, lk), y)
    loss.backward()
    assert seen == [(16, 100, torch.float32, True)]
    assert (loss.grad_fn.name() == "_DistillFnBackward") == pays
    lc, gsc, gkc = _run(HF.distillation_loss_composed, s, k, t, y, **kw)
    _check_loss(f"route-{pays}", loss.detach(), lc, l64)
    _check_grad(f"route-{pays}", "grad_s", ls.grad, gsc, gs64, torch.float32)
    _check_grad(f"route-{pays}", "grad_k", lk.grad, gkc, gk64, torch.float32)
    assert crit.bad_labels() == 0


def test_soft_cross_entropy_and_unknown_criterion():
    s, k, t, y = R.make_inputs(32, 3, "float32", 91, device=DEV)
    lk = _leaf(k)
    got = HF.soft_cross_entropy(lk, t, 2.0, route="launch")
    want = (-torch.softmax(t.double() / 2, -1) * torch.log_softmax(k.double() / 2, -1)).mean()
    _check_loss("soft_ce", got.detach(), None, want)
    got.backward()
    g64 = R.restate(None, k, t, None, base="none", kd="soft_ce", alpha=1.0, tau=2.0)[2]
    _check_grad("soft_ce", "grad", lk.grad, None, g64, torch.float32)
    # a criterion the module does not recognise is called as it is; only the KD term is the launch
    w = torch.linspace(0.5, 1.5, 3, device=DEV)
    crit = L.DistillationLoss(torch.nn.CrossEntropyLoss(weight=w), lambda inp: t, "soft", 0.25, 2.0)
    ls, lk = _leaf(s), _leaf(k)
    loss = crit(None, (ls, lk), y)
    loss.backward()
    base = torch.nn.functional.cross_entropy(s.double(), y, weight=w.double())
    kd = R.restate(None, k, t, None, base="none", kd="soft", alpha=1.0, tau=2.0)
    want = 0.75 * base + 0.25 * kd[0]
    # the base term is torch's own float32 weighted cross entropy over 32 rows of 3 classes: a handful of float32
    # roundings per row, 1e-6 is eight units of float32; the KD gradient is the launch's alone
    assert abs(float(loss.detach()) - float(want)) <= 1e-6 * float(want)
    _check_grad("own-criterion", "grad_k", lk.grad, None, 0.25 * kd[2], torch.float32)
    assert ls.grad is not None and float(ls.grad.abs().max()) > 0
