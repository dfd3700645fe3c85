"""csrc/dwbn.hip on the device: the launch (`route="launch"`) against the float64 restatement of tests/_mobilenet_ref.py,
with the composed torch route in the same input type as the yardstick -- the rule of tests/test_gpu_bnact.py, unchanged.
With e_f the launch's error and e_c the composed route's, both against float64 on the same (already rounded) inputs, and
u one unit of the delivered type (2^-23 float32, 2^-8 bfloat16, 2^-11 float16):

    y              max |err| / A elementwise,  A = |gamma| (conv(|x|; |w|) + |mean|) rstd + |beta|         e_f <= 2 max(e_c, u)
                   (eval mode: A = |a| conv(|x|; |w|) + |b| of the folded formula)
    stats,         max |err| / max |float64 value| per quantity: mean, rstd, running_mean, running_var    e_f <= 2 max(e_c, u)
    running stats  (the composed route's mean and rstd are those `torch.native_batch_norm` saves for its own z)
    dx, dw,        max |err| / max |float64 gradient|                                                     e_f <= 2 max(e_c, u)
    dgamma, dbeta  against the float64 gradient whose mask is 0 < y < 6 of that route's own stored y: the rounding of y is
                   judged once, in the forward, and no element is left out.  A float64 gradient that is exactly zero
                   (dx and dw under a zero gamma, dx under a zero filter) has no max norm: there the scale is
                   max |g| max(1, |gamma|), the scale tests/test_gpu_bnact.py uses.

Inputs: x ~ N(0, 1), w ~ N(0, 1) / 3, gamma = 2 + 0.3 N(0, 1), beta = 3 + 0.2 N(0, 1): the pre-activation is about
3 + 2 N(0, 1), so about 13 % of the outputs are clipped, half at either end, and both clamps and both mask edges are
exercised.  Every shape with at least 24 output values per channel is asserted to hold some y == 0, some y == 6 and some
strictly between; the two-value shapes exercise only the statistics.

Every case prints both errors (run with -s to see them); DESIGN.md section 25 quotes the worst."""

import pytest
import torch
import torch.nn.functional as F

import _mobilenet_ref as R
from tadmm import _cabi, ops
from tadmm import functional as HF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UNIT = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def long_shape(stride):
    """The smallest of a few candidate shapes in which, by the plan, one workgroup owns more than one band of a plane
    and more than one image: the plane is wider than a third of the staged tile, so it is cut into bands, and with 1024
    channels a channel has one workgroup."""
    for h in range(2, 9):
        shape = (2, 1024, h, 1022)
        p = ops.dwbn_plan(*shape, stride)
        if p["NB"] > 1 and p["per"] > p["NB"] and p["G"] == 1:
            return shape
    raise AssertionError("no candidate shape has a workgroup with several bands and several images")


LONG = {1: long_shape(1), 2: long_shape(2)}
SHAPES = [(2, 1, 1, 1), (2, 3, 1, 2), (3, 5, 7, 7), (2, 16, 8, 8), (4, 8, 3, 5), (2, 960, 2, 2), (64, 2, 8, 8),
          (1, 2, 112, 112), (2, 3, 33, 70), "long"]


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


def make_inputs(shape, stride, seed, kind="normal"):
    """x, w, gamma, beta, the upstream gradient and running statistics (float32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    n, c, h, wd = shape
    x = torch.randn(shape, generator=g)
    w = torch.randn(c, 1, 3, 3, generator=g) / 3
    gamma, beta = 2 + 0.3 * torch.randn(c, generator=g), 3 + 0.2 * torch.randn(c, generator=g)
    up = torch.randn((n, c) + R.out_hw(h, wd, stride), generator=g)
    rm, rv = torch.randn(c, generator=g), 0.5 + torch.rand(c, generator=g)
    if kind == "zero_filter":                          # z is constant: the variance is exactly 0 and y = clamp(beta)
        w = torch.zeros_like(w)
    elif kind == "zero_gamma":
        gamma = torch.zeros(c)
    elif kind == "offset":                             # mean 1e3, deviation 1e-2
        x = 1000 + 0.01 * x
    return x, w, gamma, beta, up, rm, rv


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


def run_route(route, x, w, gamma, beta, up, rm, rv, stride, grads, momentum=0.1):
    """One training call: y, the updated running statistics, [dx, dw, dgamma, dbeta]."""
    leaves = [t.detach().requires_grad_(grads) for t in (x, w, gamma, beta)]
    assert leaves[0].data_ptr() == x.data_ptr()
    rm_, rv_, nbt = rm.clone(), rv.clone(), torch.tensor(5, device=DEV)
    y = HF.depthwise_bn_relu6(leaves[0], leaves[1], rm_, rv_, leaves[2], leaves[3], stride=stride, training=True,
                              momentum=momentum, num_batches_tracked=nbt, route=route)
    assert y.shape == up.shape and y.dtype == x.dtype and int(nbt) == 6
    assert route == "composed" or y.is_contiguous()
    got = list(torch.autograd.grad(y, leaves, up)) if grads else [None] * 4
    return y.detach(), rm_, rv_, got


def compare(tag, x, w, gamma, beta, up, rm, rv, dtype, stride, grads=True, ref=None, clipped=False):
    """Both routes against float64 under the rule of the module docstring; returns the launch's errors."""
    n, c = x.shape[:2]
    ref = ref or R.stage(x, w, gamma, beta, stride)
    M = n * ref["z"].shape[2] * ref["z"].shape[3]
    ref_rm, ref_rv = R.running(rm, rv, ref["mean"], ref["var"], M)
    natural = float(up.abs().max()) * max(1.0, float(gamma.abs().max()))
    err = {}
    for route in ("launch", "composed"):
        y, rm_, rv_, got = run_route(route, x, w, gamma, beta, up, rm, rv, stride, grads)
        if clipped:                                    # both clamps and both mask edges are exercised
            assert int((y == 0).sum()) > 0 and int((y == 6).sum()) > 0 and int(((y > 0) & (y < 6)).sum()) > 0, tag
        e = {"y": float(((R.f64(y) - ref["y"]).abs() / ref["A"].clamp_min(1e-300)).max()),
             "running_mean": max_err(rm_, ref_rm), "running_var": max_err(rv_, ref_rv)}
        if route == "launch":
            _, _, stats = ops.dwbn_fwd(x, w, gamma, beta, None, None, stride=stride, training=True, need_stats=True)
            mean, rstd = stats[:, 0], stats[:, 1]
        else:
            zc = F.conv2d(x, w.to(x.dtype), None, stride, 1, 1, c)
            _, mean, rstd = torch.native_batch_norm(zc, gamma.to(x.dtype), beta.to(x.dtype), None, None, True, 0.1, 1e-5)
        e["mean"] = max_err(mean, ref["mean"], float(ref["z"].abs().max()))
        e["rstd"] = max_err(rstd, ref["rstd"])
        if grads:
            want = R.stage_grads(x, w, gamma, beta, stride, up, (y > 0) & (y < 6), st=ref)
            for i, name in enumerate(("dx", "dw", "dgamma", "dbeta")):
                assert got[i].dtype == (x, w, gamma, beta)[i].dtype and got[i].shape == (x, w, gamma, beta)[i].shape
                e[name] = max_err(got[i], want[name], natural)
        err[route] = e
    return {k: bar(err["launch"][k], err["composed"][k], dtype, f"{tag} {k}") for k in err["launch"]}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("stride", [1, 2], ids=["s1", "s2"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s if isinstance(s, str) else "x".join(str(v) for v in s) for s in SHAPES])
def test_forward_and_backward_against_float64(shape, stride, dtype):
    shape = LONG[stride] if shape == "long" else shape
    x, w, gamma, beta, up, rm, rv = make_inputs(shape, stride, seed=sum(shape) + stride)
    w, gamma, beta, rm, rv, up = (t.to(DEV) for t in (w, gamma, beta, rm, rv, up.to(dtype)))
    ref = R.stage(x.to(dtype), w, gamma, beta, stride)                # the same rounded inputs for both layouts
    ho, wo = ref["z"].shape[2:]
    clipped = shape[0] * ho * wo >= 24
    if clipped:
        y = ref["y"]
        assert int((y == 0).sum()) > 0 and int((y == 6).sum()) > 0 and int(((y > 0) & (y < 6)).sum()) > 0
    for layout in ("plain", "odd"):
        compare(f"x={layout}", place(x, layout, dtype), w, gamma, beta, up, rm, rv, dtype, stride, ref=ref, clipped=clipped)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["zero_filter", "zero_gamma", "offset"])
def test_hard_channels(kind, dtype):
    for shape, stride in (((3, 5, 7, 7), 1), ((2, 16, 8, 8), 2), ((64, 2, 8, 8), 1)):
        x, w, gamma, beta, up, rm, rv = make_inputs(shape, stride, seed=31 + shape[1], kind=kind)
        w, gamma, beta, rm, rv, up = (t.to(DEV) for t in (w, gamma, beta, rm, rv, up.to(dtype)))
        e = compare(f"{kind} {shape} s{stride}", place(x, "plain", dtype), w, gamma, beta, up, rm, rv, dtype, stride)
        if kind == "zero_filter":                      # z == 0: the variance is exactly 0, y = clamp(beta), dx exact zeros
            y, _, _, got = run_route("launch", place(x, "plain", dtype), w, gamma, beta, up, rm, rv, stride, True)
            want = beta.clamp(0, 6).to(dtype)[None, :, None, None].expand_as(y)
            assert torch.equal(y, want) and e["dx"] == 0.0 and int(got[0].ne(0).sum()) == 0
            _, _, stats = ops.dwbn_fwd(place(x, "plain", dtype), w, gamma, beta, None, None, stride=stride, training=True,
                                       need_stats=True)
            assert float(stats[:, 0].abs().max()) == 0.0
            assert torch.equal(stats[:, 1], torch.full_like(stats[:, 1], 1.0 / (1e-5 ** 0.5)))
        if kind == "zero_gamma":
            assert e["dx"] == 0.0 and e["dw"] == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_eval_mode_is_the_folded_formula(dtype):
    for shape, stride in (((3, 5, 7, 7), 1), ((3, 5, 7, 7), 2), ((2, 16, 8, 8), 1), ((2, 16, 8, 8), 2), ((1, 3, 1, 1), 1),
                          ((1, 2, 112, 112), 2), ((2, 3, 33, 70), 1)):
        x, w, gamma, beta, up, rm, rv = make_inputs(shape, stride, seed=shape[1])
        w, gamma, beta, rm, rv = (t.to(DEV) for t in (w, gamma, beta, rm, rv))
        for layout in ("plain", "odd"):
            xd = place(x, layout, dtype)
            want, scale = R.stage_eval(xd, w, rm, rv, gamma, beta, stride)
            e = {}
            for route in ("launch", "composed"):
                rm_, rv_, nbt = rm.clone(), rv.clone(), torch.tensor(5, device=DEV)
                with torch.no_grad():
                    y = HF.depthwise_bn_relu6(xd, w, rm_, rv_, gamma, beta, stride=stride, training=False,
                                              num_batches_tracked=nbt, route=route)
                assert torch.equal(rm_, rm) and torch.equal(rv_, rv) and int(nbt) == 5     # eval touches nothing
                assert y.shape == want.shape and y.dtype == dtype
                e[route] = float(((R.f64(y) - want).abs() / scale.clamp_min(1e-300)).max())
            bar(e["launch"], e["composed"], dtype, f"eval {shape} s{stride} x={layout}")


def test_float16_is_forward_only():
    dtype = torch.float16
    for shape, stride in (((3, 5, 7, 7), 1), ((2, 16, 8, 8), 2), ((64, 2, 8, 8), 1)):
        x, w, gamma, beta, up, rm, rv = make_inputs(shape, stride, seed=3)
        w, gamma, beta, rm, rv, up = (t.to(DEV) for t in (w, gamma, beta, rm, rv, up.to(dtype)))
        for layout in ("plain", "odd"):
            with torch.no_grad():
                compare(f"f16 {shape} s{stride} {layout}", place(x, layout, dtype), w, gamma, beta, up, rm, rv, dtype, stride,
                        grads=False)
    xd = place(x, "plain", dtype)
    y, z, stats = ops.dwbn_fwd(xd, w, gamma, beta, rm.clone(), rv.clone(), stride=stride, training=True, need_stats=True)
    with pytest.raises(_cabi.TadmmError, match="forward only"):
        ops.dwbn_bwd(up, y, z, xd, w, gamma, stats, stride=stride)
    with pytest.raises(_cabi.TadmmError, match="float16 with gradients"):
        HF.depthwise_bn_relu6(xd.requires_grad_(), w, rm, rv, gamma, beta, stride=stride, training=True, route="launch")
    # left alone, the call is composed: it is differentiable and equals the composed route bit for bit
    got = HF.depthwise_bn_relu6(xd, w, rm.clone(), rv.clone(), gamma, beta, stride=stride, training=True)
    want = HF.depthwise_bn_relu6_composed(xd, w, rm.clone(), rv.clone(), gamma, beta, stride=stride, training=True)
    assert got.grad_fn is not None and torch.equal(got, want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_two_runs_are_bit_identical_and_the_counter_counts(dtype):
    for shape, stride in (((1, 2, 112, 112), 1), ((64, 3, 8, 8), 2), ((5, 600, 9, 11), 1)):
        x, w, gamma, beta, up, rm, rv = make_inputs(shape, stride, seed=5)
        xd = place(x, "plain", dtype)
        w, gamma, beta, rm, rv, up = (t.to(DEV) for t in (w, gamma, beta, rm, rv, up.to(dtype)))
        other = make_inputs((3, 5, 7, 7), 1, seed=6)
        runs = []
        nbt = torch.tensor(0, device=DEV)
        for n in range(2):
            leaves = [t.detach().requires_grad_() for t in (xd, w, gamma, beta)]
            rm_, rv_ = rm.clone(), rv.clone()
            y = HF.depthwise_bn_relu6(*leaves[:2], rm_, rv_, *leaves[2:], stride=stride, training=True,
                                      num_batches_tracked=nbt, route="launch")
            assert int(nbt) == n + 1
            runs.append((y, rm_, rv_) + torch.autograd.grad(y, leaves, up))
            if n == 0:                                 # a call of another shape in between
                o = [t.to(DEV) for t in other]
                HF.depthwise_bn_relu6(o[0].requires_grad_(), o[1], o[5], o[6], o[2], o[3], stride=1, training=True,
                                      route="launch").sum().backward()
        for a, c in zip(*runs):
            assert torch.equal(a, c)
        with torch.no_grad():
            HF.depthwise_bn_relu6(xd, w, rm, rv, gamma, beta, stride=stride, training=False, num_batches_tracked=nbt,
                                  route="launch")
        assert int(nbt) == 2
    # what the launch does not take raises under route="launch" before anything runs (tests/test_dwbn_host_cpu.py
    # follows the same calls to the composed route under route=None)
    with pytest.raises(_cabi.TadmmError, match="NCHW contiguous"):
        HF.depthwise_bn_relu6(xd.transpose(2, 3), w, rm.clone(), rv.clone(), gamma, beta, stride=1, training=True, route="launch")
    with pytest.raises(_cabi.TadmmError, match="momentum=None"):
        HF.depthwise_bn_relu6(xd, w, rm.clone(), rv.clone(), gamma, beta, stride=1, training=True, momentum=None, route="launch")
    with pytest.raises(_cabi.TadmmError, match="padding"):
        HF.depthwise_bn_relu6(xd, w, rm.clone(), rv.clone(), gamma, beta, stride=1, padding=0, training=True, route="launch")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_nullable_outputs_equal_the_full_call(dtype):
    for shape, stride in (((3, 5, 7, 7), 2), ((2, 16, 8, 8), 1), ((1, 2, 112, 112), 2), ((5, 600, 9, 11), 1)):
        x, w, gamma, beta, up, rm, rv = make_inputs(shape, stride, seed=9)
        xd = place(x, "plain", dtype)
        w, gamma, beta, up = (t.to(DEV) for t in (w, gamma, beta, up.to(dtype)))
        y, z, stats = ops.dwbn_fwd(xd, w, gamma, beta, None, None, stride=stride, training=True, need_stats=True)
        full = ops.dwbn_bwd(up, y, z, xd, w, gamma, stats, stride=stride)
        for i in range(4):
            need = tuple(j == i for j in range(4))
            got = ops.dwbn_bwd(up, y, z, xd, w, gamma, stats, stride=stride, need=need)
            assert all((got[j] is None) == (j != i) for j in range(4))
            assert torch.equal(got[i], full[i]), (shape, stride, i)
        assert ops.dwbn_bwd(up, y, z, xd, w, gamma, stats, stride=stride, need=(False,) * 4) == (None,) * 4
