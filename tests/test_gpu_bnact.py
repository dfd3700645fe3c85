"""csrc/bnact.hip on the device: the launch (`route="launch"`) against the float64 restatement of tests/_resnet_ref.py,
with the composed torch route in the same input type as the yardstick -- the rule of tests/test_gpu_prenorm.py.  With e_f
the launch's error and e_c the composed route's, both against float64 on the same (already rounded) inputs, and u one
unit of the delivered type (2^-23 float32, 2^-8 bfloat16, 2^-11 float16):

    y              max |err| / A elementwise,  A = |gamma| (|x| + |mean|) rstd + |beta| + |res|           e_f <= 2 max(e_c, u)
                   (eval mode: A = |a x| + |b| + |res| of the folded formula)
    stats,         max |err| / max |float64 value| per quantity: mean, rstd, running_mean, running_var    e_f <= 2 max(e_c, u)
    running stats  (the composed route's mean and rstd are those `torch.native_batch_norm` saves)
    dx, dres,      max |err| / max |float64 gradient|                                                     e_f <= 2 max(e_c, u)
    dgamma, dbeta  against the float64 gradient whose ReLU mask is that route's own stored y: the rounding of y is judged
                   once, in the forward, and no element is left out.  A float64 gradient that is exactly zero (y == 0
                   everywhere, dx under a zero gamma) has no max norm: there the scale is max |g| max(1, |gamma|).

Every case prints both errors (run with -s to see them); DESIGN.md section 24 quotes the worst."""
import pytest
import torch

import _resnet_ref as R
from tadmm import _cabi, ops
from tadmm import functional as HF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UNIT = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# the splits of a one-channel tensor this large (the cap of the split), and a shape in which each of them owns more than
# two trips of the widest trip (2048 values): a workgroup walks its span in several steps
SPLITS = ops.bnact_workspace_bytes(9, 1, 256, 257) // 16
LONG = (9, 1, 256, 257)
assert LONG[0] * LONG[2] * LONG[3] > 2 * 2048 * SPLITS

SHAPES = [(2, 1, 1, 1), (1, 3, 1, 2), (3, 5, 7, 7), (2, 16, 8, 8), (4, 8, 3, 5), (2, 64, 1, 1), (64, 2, 32, 32),
          (2, 2048, 7, 7), LONG]
# (layout of x, residual, layout of the residual, relu)
VARIANTS = [("plain", None, None, True), ("odd", None, None, False), ("plain", "full", "plain", True),
            ("odd", "full", "plain", False), ("plain", "full", "odd", True)]


def place(t, layout, dtype):
    """A CPU float32 tensor on the device in `dtype`: as it is, or starting one element into its allocation."""
    t = t.to(dtype)
    if layout != "odd":
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=dtype, device=DEV)
    buf[1:].copy_(t.reshape(-1))
    v = buf[1:].view(t.shape)
    assert (v.data_ptr() // v.element_size()) % 2 == 1 and v.is_contiguous()
    return v


def make_inputs(shape, seed, kind="normal"):
    """x, gamma, beta, a full-width residual, the upstream gradient and running statistics (float32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    c = shape[1]
    x = 0.5 + 2 * torch.randn(shape, generator=g)
    gamma, beta = 1 + 0.5 * torch.randn(c, generator=g), torch.randn(c, generator=g)
    res, up = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    rm, rv = torch.randn(c, generator=g), 0.5 + torch.rand(c, generator=g)
    if kind == "constant":                             # the variance is 0
        x = torch.full(shape, 2.5)
    elif kind == "offset":                             # mean / std around 1e5
        x = 1000 + 0.01 * x
    elif kind == "negative":                           # every pre-activation below zero: y == 0, the gradients exact zeros
        beta, res = -100 - beta.abs(), -res.abs()
    elif kind == "zero_gamma":
        gamma = torch.zeros(c)
    return x, gamma, beta, res, up, rm, rv


def max_err(got, want, natural=None):
    scale = float(want.abs().max()) or (natural or 0.0)
    err = float((got.detach().to("cpu", torch.float64).reshape(want.shape) - want).abs().max())
    if scale == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / scale


def bar(e_f, e_c, dtype, what):
    print(f"    {what:<52s} launch {e_f:.3e}   composed {e_c:.3e}   unit {UNIT[dtype]:.3e}")
    assert e_f <= 2.0 * max(e_c, UNIT[dtype]), (what, e_f, e_c)
    return e_f


def run_route(route, x, gamma, beta, res, c0, up, rm, rv, relu, grads, momentum=0.1):
    """One training call: y, the updated running statistics and counter, [dx, dgamma, dbeta, dres]."""
    leaves = [t.detach().requires_grad_(grads) for t in (x, gamma, beta)] + \
        ([] if res is None else [res.detach().requires_grad_(grads)])
    assert leaves[0].data_ptr() == x.data_ptr() and (res is None or leaves[3].data_ptr() == res.data_ptr())
    rm_, rv_, nbt = rm.clone(), rv.clone(), torch.tensor(5, device=DEV)
    y = HF.batch_norm_act(leaves[0], rm_, rv_, leaves[1], leaves[2], None if res is None else leaves[3],
                          res_channel_offset=c0, training=True, momentum=momentum, relu=relu, num_batches_tracked=nbt,
                          route=route)
    assert y.shape == x.shape and y.dtype == x.dtype and int(nbt) == 6
    assert route == "composed" or y.is_contiguous()
    got = list(torch.autograd.grad(y, leaves, up)) if grads else [None] * len(leaves)
    return y.detach(), rm_, rv_, got


def compare(tag, x, gamma, beta, res, c0, up, rm, rv, dtype, relu, grads=True):
    """Both routes against float64 under the rule of the module docstring; returns the launch's errors."""
    n, c, h, w = x.shape
    ref = R.tail(x, gamma, beta, res, c0, relu)
    ref_rm, ref_rv = R.running(rm, rv, ref["mean"], ref["var"], n * h * w)
    natural = float(up.abs().max()) * max(1.0, float(gamma.abs().max()))
    err = {}
    for route in ("launch", "composed"):
        y, rm_, rv_, got = run_route(route, x, gamma, beta, res, c0, up, rm, rv, relu, grads)
        e = {"y": float(((R.f64(y) - ref["y"]).abs() / ref["A"].clamp_min(1e-300)).max()),
             "running_mean": max_err(rm_, ref_rm), "running_var": max_err(rv_, ref_rv)}
        if route == "launch":
            _, stats = ops.bnact_fwd(x, gamma, beta, None, None, res, c0=c0, training=True, relu=relu, need_stats=True)
            mean, rstd = stats[:, 0], stats[:, 1]
        else:
            _, mean, rstd = torch.native_batch_norm(x, gamma.to(x.dtype), beta.to(x.dtype), None, None, True, 0.1, 1e-5)
        e["mean"] = max_err(mean, ref["mean"], float(R.f64(x).abs().max()))
        e["rstd"] = max_err(rstd, ref["rstd"])
        if grads:
            want = R.tail_grads(x, gamma, beta, res, c0, up, (y > 0) if relu else None)
            for i, name in enumerate(("dx", "dgamma", "dbeta") + (() if res is None else ("dres",))):
                assert got[i].dtype == ((x, gamma, beta) + (() if res is None else (res,)))[i].dtype
                e[name] = max_err(got[i], want[name], natural)
        err[route] = e
    return {k: bar(err["launch"][k], err["composed"][k], dtype, f"{tag} {k}") for k in err["launch"]}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(str(v) for v in s) for s in SHAPES])
def test_forward_and_backward_against_float64(shape, dtype):
    x, gamma, beta, res, up, rm, rv = make_inputs(shape, seed=sum(shape))
    gamma, beta, rm, rv, up = gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV), up.to(dtype).to(DEV)
    for xl, rk, rl, relu in VARIANTS:
        compare(f"x={xl} res={rk}/{rl} relu={int(relu)}", place(x, xl, dtype), gamma, beta,
                None if rk is None else place(res, rl, dtype), 0, up, rm, rv, dtype, relu)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [((2, 8, 8, 8), 16, 4), ((2, 4, 7, 7), 8, 2)], ids=["8x8-into-16", "7x7-into-8"])
def test_option_a_window(case, dtype):
    """The shortcut of resnet_cifar_tt.py: x_in[:, :, ::2, ::2] added to the channels [c0, c0 + Cr), read through its
    strides; its gradient is the masked gradient over the window and an exact nothing elsewhere."""
    in_shape, c, c0 = case
    n, cr, hi, wi = in_shape
    shape = (n, c, (hi + 1) // 2, (wi + 1) // 2)
    x, gamma, beta, _, up, rm, rv = make_inputs(shape, seed=c)
    x_in = torch.randn(in_shape, generator=torch.Generator().manual_seed(c0))
    gamma, beta, rm, rv, up = gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV), up.to(dtype).to(DEV)
    for xl, rl, relu in (("plain", "plain", True), ("odd", "odd", True), ("plain", "odd", False)):
        base = place(x_in, rl, dtype)
        view = base[:, :, ::2, ::2]
        assert view.shape == (n, cr, shape[2], shape[3]) and view.data_ptr() == base.data_ptr() and not view.is_contiguous()
        compare(f"optionA x={xl} res={rl} relu={int(relu)}", place(x, xl, dtype), gamma, beta, view, c0, up, rm, rv, dtype, relu)
    # through the base tensor: autograd carries the window's gradient back through the strided view
    base = place(x_in, "plain", dtype).requires_grad_()
    xd = place(x, "plain", dtype).requires_grad_()
    outs = []
    for route in ("launch", "composed"):
        y = HF.batch_norm_act(xd, rm.clone(), rv.clone(), gamma, beta, base[:, :, ::2, ::2], res_channel_offset=c0,
                              training=True, route=route)
        outs.append(torch.autograd.grad(y, base, up)[0])
    assert outs[0].shape == base.shape and float(outs[0][:, :, 1::2].abs().max()) == 0.0
    assert float((outs[0].float() - outs[1].float()).abs().max()) <= 4 * UNIT[dtype] * float(outs[1].abs().max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["constant", "offset", "negative", "zero_gamma"])
def test_hard_channels(kind, dtype):
    for shape in ((3, 5, 7, 7), (2, 16, 8, 8), (64, 2, 32, 32)):
        x, gamma, beta, res, up, rm, rv = make_inputs(shape, seed=31 + shape[1], kind=kind)
        args = [t.to(DEV) for t in (gamma, beta)]
        e = compare(f"{kind} {shape}", place(x, "plain", dtype), *args, place(res, "plain", dtype), 0,
                    up.to(dtype).to(DEV), rm.to(DEV), rv.to(DEV), dtype, True)
        if kind == "negative":                         # y == 0: exact zeros, not small numbers
            assert all(e[k] == 0.0 for k in ("dx", "dgamma", "dbeta", "dres"))
            y, _, _, got = run_route("launch", place(x, "plain", dtype), *args, place(res, "plain", dtype), 0,
                                     up.to(dtype).to(DEV), rm.to(DEV), rv.to(DEV), True, True)
            assert int(y.ne(0).sum()) == 0 and all(int(t.ne(0).sum()) == 0 for t in got)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_eval_mode_is_the_folded_formula(dtype):
    for shape, c0, cr in (((3, 5, 7, 7), 0, 5), ((2, 16, 8, 8), 4, 8), ((1, 3, 1, 1), 1, 1), ((2, 2048, 7, 7), 0, 2048)):
        x, gamma, beta, res, up, rm, rv = make_inputs(shape, seed=shape[1])
        gamma, beta, rm, rv = gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV)
        for xl, rl, relu, with_res in (("plain", "plain", True, True), ("odd", "odd", False, True), ("plain", None, True, False)):
            xd = place(x, xl, dtype)
            rd = place(res[:, :cr].contiguous(), rl, dtype) if with_res else None
            want, scale = R.tail_eval(xd, rm, rv, gamma, beta, rd, c0 if with_res else 0, relu)
            e = {}
            for route in ("launch", "composed"):
                rm_, rv_, nbt = rm.clone(), rv.clone(), torch.tensor(5, device=DEV)
                with torch.no_grad():
                    y = HF.batch_norm_act(xd, rm_, rv_, gamma, beta, rd, res_channel_offset=c0 if with_res else 0,
                                          training=False, relu=relu, num_batches_tracked=nbt, route=route)
                assert torch.equal(rm_, rm) and torch.equal(rv_, rv) and int(nbt) == 5     # eval touches nothing
                e[route] = float(((R.f64(y) - want).abs() / scale.clamp_min(1e-300)).max())
            bar(e["launch"], e["composed"], dtype, f"eval {shape} x={xl} res={rl} relu={int(relu)}")


def test_float16_is_forward_only():
    dtype = torch.float16
    for shape in ((3, 5, 7, 7), (2, 16, 8, 8), (64, 2, 32, 32)):
        x, gamma, beta, res, up, rm, rv = make_inputs(shape, seed=3)
        gamma, beta, rm, rv, up = gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV), up.to(dtype).to(DEV)
        for xl, rl in (("plain", "plain"), ("odd", "odd")):
            with torch.no_grad():
                compare(f"f16 {shape} {xl}", place(x, xl, dtype), gamma, beta, place(res, rl, dtype), 0, up, rm, rv, dtype,
                        True, grads=False)
    xd = place(x, "plain", dtype)
    y, stats = ops.bnact_fwd(xd, gamma, beta, rm.clone(), rv.clone(), training=True, need_stats=True)
    with pytest.raises(_cabi.TadmmError, match="forward only"):
        ops.bnact_bwd(up, y, xd, gamma, stats)
    with pytest.raises(_cabi.TadmmError, match="float16 with gradients"):
        HF.batch_norm_act(xd.requires_grad_(), rm, rv, gamma, beta, training=True, route="launch")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_two_runs_are_bit_identical_and_the_counter_counts(dtype):
    shape = LONG[:1] + (3,) + LONG[2:]                 # every split of a channel owns several trips
    x, gamma, beta, res, up, rm, rv = make_inputs(shape, seed=5)
    xd, rd, up = place(x, "plain", dtype), place(res, "plain", dtype), up.to(dtype).to(DEV)
    gamma, beta, rm, rv = gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV)
    other = make_inputs((3, 5, 7, 7), seed=6)
    runs = []
    nbt = torch.tensor(0, device=DEV)
    for n in range(2):
        leaves = [t.detach().requires_grad_() for t in (xd, gamma, beta, rd)]
        rm_, rv_ = rm.clone(), rv.clone()
        y = HF.batch_norm_act(leaves[0], rm_, rv_, leaves[1], leaves[2], leaves[3], training=True, num_batches_tracked=nbt,
                              route="launch")
        assert int(nbt) == n + 1
        runs.append((y, rm_, rv_) + torch.autograd.grad(y, leaves, up))
        if n == 0:                                     # a call of another shape in between
            o = [t.to(DEV) for t in other]
            HF.batch_norm_act(o[0].requires_grad_(), o[5], o[6], o[1], o[2], o[3], training=True, route="launch").sum().backward()
    for a, c in zip(*runs):
        assert torch.equal(a, c)
    with torch.no_grad():
        HF.batch_norm_act(xd, rm, rv, gamma, beta, training=False, num_batches_tracked=nbt, route="launch")
    assert int(nbt) == 2
    # what the launch does not take raises under route="launch" before anything runs (tests/test_bnact_host_cpu.py
    # follows the same calls to the composed route under route=None)
    xcl = xd[:2].contiguous(memory_format=torch.channels_last)
    with pytest.raises(_cabi.TadmmError, match="NCHW contiguous"):
        HF.batch_norm_act(xcl, rm.clone(), rv.clone(), gamma, beta, training=True, route="launch")
    with pytest.raises(_cabi.TadmmError, match="momentum=None"):
        HF.batch_norm_act(xd, rm.clone(), rv.clone(), gamma, beta, training=True, momentum=None, route="launch")
