"""The ownership branches of csrc/bnact.hip, csrc/dwbn.hip and csrc/densebn.hip on the device, each against float64.

tests/_bn_ownership.py names the branches of the three planners that production batch sizes take -- several images in
one staged tile (dwbn: G > 1, short last groups, G stopped by the tile, by the output cap, by N / want), a split walked
in several steps that cross planes (bnact, densebn: step_q >= 1, with and without a remainder, a partial last trip),
more than 64 splits, statistics launches that plan another split than their consumer -- and resolves each to a shape
through the library's plan queries; tests/test_bn_ownership_host_cpu.py checks that on the CPU.  This file runs them.

Nothing is judged by a rule of its own: `compare`, `make_inputs`, `place` and `bar` are those of
tests/test_gpu_bnact.py, tests/test_gpu_dwbn.py and tests/test_gpu_densebn.py, so the rule stays e_f <= 2 max(e_c, u)
for y, mean, rstd, the running statistics and every gradient, against the float64 restatements of _resnet_ref.py,
_mobilenet_ref.py and _densenet_ref.py, with the composed torch route in the same type as the yardstick.  On top of
that every dwbn shape asserts that a single requested gradient equals the full call's bit for bit, and every shape is
run twice for bit identity.  Every case prints both errors (run with -s); DESIGN.md quotes the worst per kernel."""
import contextlib
import functools

import pytest
import torch

import _bn_ownership as B
import _densenet_ref as RD
import _mobilenet_ref as RM
import test_gpu_bnact as TB
import test_gpu_densebn as TN
import test_gpu_dwbn as TD
from tadmm import functional as HF
from tadmm import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TRAIN = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
ALL = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])


def slug(name):
    return name.replace(", ", ",").replace(" ", "-")


DW_CASES = pytest.mark.parametrize("name,stride", B.DWBN_CASES, ids=[f"{slug(n)}-s{s}" for n, s in B.DWBN_CASES])
BA_NAMES = pytest.mark.parametrize("name", [b[0] for b in B.BNACT], ids=[slug(b[0]) for b in B.BNACT])
DB_NAMES = pytest.mark.parametrize("name", [b[0] for b in B.DENSEBN], ids=[slug(b[0]) for b in B.DENSEBN])


def same_bits(first, second, tag):
    for a, b in zip(first, second):
        if isinstance(a, (list, tuple)):
            same_bits(a, b, tag)
        else:
            assert (a is None and b is None) or torch.equal(a, b), tag


# ------------------------------------------------------------------------------------------------------------ dwbn
@functools.lru_cache(maxsize=2)
def dwbn_inputs(shape, stride):
    """The CPU float32 inputs of a shape, made once and left unchanged."""
    return TD.make_inputs(shape, stride, seed=B.dwbn_seed(shape, stride))


def yardstick(case, dtype):
    """The composed route is the yardstick as it is, with one exception of speed: the weight gradient of a 16-bit
    depthwise convolution whose output plane is 1 x 1 takes MIOpen 0.09 s per image on the MI355X (42 s for the 460
    images the all-halo branch needs, whatever C is).  There F.conv2d runs on torch's own depthwise kernels -- the same
    composed route in the same type, 0.1 s."""
    if B.ES[dtype] == 2 and case["Ho"] * case["Wo"] == 1:
        return torch.backends.cudnn.flags(enabled=False)
    return contextlib.nullcontext()


@TRAIN
@DW_CASES
def test_dwbn_branch_against_float64(name, stride, dtype):
    case = B.dwbn(name, stride, dtype)
    shape, layout = case["shape"], case["layout"]
    print(f"\n  dwbn {name}: {shape} s{stride} x={layout} wide={int(case['wide'])} "
          + " ".join(f"{k}={case[k]}" for k in ("G", "RB", "NB", "U", "S", "per")))
    x, w, gamma, beta, up, rm, rv = dwbn_inputs(shape, stride)
    w, gamma, beta, rm, rv, up = (t.to(DEV) for t in (w, gamma, beta, rm, rv, up.to(dtype)))
    ref = RM.stage(x.to(dtype), w, gamma, beta, stride)
    y = ref["y"]
    assert int((y == 0).sum()) > 0 and int((y == 6).sum()) > 0 and int(((y > 0) & (y < 6)).sum()) > 0
    xd = TD.place(x, layout, dtype)
    with yardstick(case, dtype):
        TD.compare(f"dwbn/{slug(name)} s{stride}", xd, w, gamma, beta, up, rm, rv, dtype, stride, ref=ref, clipped=True)
    # a single requested gradient equals the full call's, bit for bit
    y, z, stats = ops.dwbn_fwd(xd, w, gamma, beta, None, None, stride=stride, training=True, need_stats=True)
    full = ops.dwbn_bwd(up, y, z, xd, w, gamma, stats, stride=stride)
    for i in range(4):
        got = ops.dwbn_bwd(up, y, z, xd, w, gamma, stats, stride=stride, need=tuple(j == i for j in range(4)))
        assert all((got[j] is None) == (j != i) for j in range(4))
        assert torch.equal(got[i], full[i]), (name, stride, i)
    # and two runs are bit-identical
    runs = [TD.run_route("launch", xd, w, gamma, beta, up, rm, rv, stride, True) for _ in range(2)]
    same_bits(*runs, (name, stride))
    assert torch.equal(runs[0][0], y) and all(torch.equal(a, b) for a, b in zip(runs[0][3], full))


@ALL
@DW_CASES
def test_dwbn_branch_eval_mode(name, stride, dtype):
    """The eval kernel shares the staging and the (g, row) indexing of the training convolution."""
    case = B.dwbn(name, stride, dtype)
    shape, layout = case["shape"], case["layout"]
    x, w, gamma, beta, _, rm, rv = dwbn_inputs(shape, stride)
    w, gamma, beta, rm, rv = (t.to(DEV) for t in (w, gamma, beta, rm, rv))
    xd = TD.place(x, layout, dtype)
    want, scale = RM.stage_eval(xd, w, rm, rv, gamma, beta, stride)
    e = {}
    for route in ("launch", "composed"):
        rm_, rv_, nbt = rm.clone(), rv.clone(), torch.tensor(5, device=DEV)
        with torch.no_grad():
            y = HF.depthwise_bn_relu6(xd, w, rm_, rv_, gamma, beta, stride=stride, training=False, num_batches_tracked=nbt,
                                      route=route)
        assert torch.equal(rm_, rm) and torch.equal(rv_, rv) and int(nbt) == 5             # eval touches nothing
        assert y.shape == want.shape and y.dtype == dtype
        e[route] = float(((RM.f64(y) - want).abs() / scale.clamp_min(1e-300)).max())
    TD.bar(e["launch"], e["composed"], dtype, f"dwbn-eval/{slug(name)} s{stride} G={case['G']}")


@DW_CASES
def test_dwbn_branch_float16_forward(name, stride):
    dtype = torch.float16
    case = B.dwbn(name, stride, dtype)
    shape, layout = case["shape"], case["layout"]
    x, w, gamma, beta, up, rm, rv = dwbn_inputs(shape, stride)
    w, gamma, beta, rm, rv, up = (t.to(DEV) for t in (w, gamma, beta, rm, rv, up.to(dtype)))
    ref = RM.stage(x.to(dtype), w, gamma, beta, stride)
    with torch.no_grad():
        TD.compare(f"dwbn-f16/{slug(name)} s{stride} G={case['G']}", TD.place(x, layout, dtype), w, gamma, beta, up, rm, rv,
                   dtype, stride, grads=False, ref=ref, clipped=True)


# ----------------------------------------------------------------------------------------------------------- bnact
@functools.lru_cache(maxsize=2)
def bnact_inputs(shape):
    return TB.make_inputs(shape, seed=sum(shape))


def describe(kernel, name, case):
    print(f"\n  {kernel} {name}: {case.get('shape', case.get('layout'))} vec={case['vec']} "
          + " ".join(f"{k}={case[k]}" for k in ("S", "span", "cap", "steps", "step_q", "step_r", "wraps", "partial")))


@TRAIN
@pytest.mark.parametrize("variant", TB.VARIANTS, ids=[f"x={v[0]}-res={v[1]}/{v[2]}-relu={int(v[3])}" for v in TB.VARIANTS])
@BA_NAMES
def test_bnact_branch_against_float64(name, variant, dtype):
    """A variant with an odd layout walks the same shape by element: the steps are a quarter or an eighth as long and
    cross planes at other positions."""
    case = B.bnact(name, dtype)
    describe("bnact", name, case)
    xl, rk, rl, relu = variant
    x, gamma, beta, res, up, rm, rv = bnact_inputs(case["shape"])
    gamma, beta, rm, rv, up = gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV), up.to(dtype).to(DEV)
    TB.compare(f"bnact/{slug(name)} x={xl} res={rk}/{rl} relu={int(relu)}", TB.place(x, xl, dtype), gamma, beta,
               None if rk is None else TB.place(res, rl, dtype), 0, up, rm, rv, dtype, relu)


@TRAIN
@BA_NAMES
def test_bnact_branch_option_a_window_and_two_runs(name, dtype):
    """The strided shortcut x_in[:, :, ::2, ::2] over a window of channels is read by element at the positions the
    several-step walk arrives at; and two runs of the full-residual call are bit-identical."""
    case = B.bnact(name, dtype)
    n, c, h, w = case["shape"]
    x, gamma, beta, res, up, rm, rv = bnact_inputs(case["shape"])
    gamma, beta, rm, rv, up = gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV), up.to(dtype).to(DEV)
    cr = min(c - 1, 8)
    c0 = (c - cr) // 2
    x_in = torch.randn((n, cr, 2 * h, 2 * w - 1), generator=torch.Generator().manual_seed(c0))
    for xl, rl, relu in (("plain", "plain", True), ("odd", "odd", False)):
        base = TB.place(x_in, rl, dtype)
        view = base[:, :, ::2, ::2]
        assert view.shape == (n, cr, h, w) and view.data_ptr() == base.data_ptr() and not view.is_contiguous()
        assert view.stride(2) != view.stride(3) * w                    # neither plane-contiguous nor linear in p
        TB.compare(f"bnact-optionA/{slug(name)} x={xl} res={rl} relu={int(relu)}", TB.place(x, xl, dtype), gamma, beta,
                   view, c0, up, rm, rv, dtype, relu)
    xd, rd = TB.place(x, "plain", dtype), TB.place(res, "plain", dtype)
    runs = [TB.run_route("launch", xd, gamma, beta, rd, 0, up, rm, rv, True, True) for _ in range(2)]
    same_bits(*runs, name)


# --------------------------------------------------------------------------------------------------------- densebn
@TRAIN
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@DB_NAMES
def test_densebn_branch_against_float64(name, relu, dtype):
    case = B.densebn(name, dtype)
    describe("densebn", name, case)
    print("  statistics plans (S, span, steps): " + str([(s["S"], s["span"], s["steps"]) for s in case["stats"]]))
    args = TN.on_device(case["layout"], dtype, seed=len(name))
    TN.compare(f"densebn/{slug(name)} relu={int(relu)}", *args, dtype, relu)
    if relu:                                            # two runs are bit-identical
        runs = [TN.run_route("launch", *args, True, True) for _ in range(2)]
        same_bits(*runs, name)


@ALL
@pytest.mark.parametrize("name", B.DENSEBN_EVAL_AND_F16, ids=[slug(n) for n in B.DENSEBN_EVAL_AND_F16])
def test_densebn_branch_eval_mode(name, dtype):
    case = B.densebn(name, dtype)
    segs, gamma, beta, up, rm, rv = TN.on_device(case["layout"], dtype, seed=7)
    for relu in (True, False):
        want = RD.pre_act_eval(segs, rm, rv, gamma, beta, relu)
        e = {}
        for route in ("launch", "composed"):
            rm_, rv_, nbt = rm.clone(), rv.clone(), torch.tensor(5, device=DEV)
            feats = HF.DenseFeatures(segs)
            with torch.no_grad():
                y = HF.dense_batch_norm_act(feats, rm_, rv_, gamma, beta, training=False, relu=relu,
                                            num_batches_tracked=nbt, route=route)
            assert torch.equal(rm_, rm) and torch.equal(rv_, rv) and int(nbt) == 5         # eval touches nothing
            assert feats._stats == [None] * len(segs)                                       # and computes no statistics
            e[route] = TN.max_err(y, want)
        TN.bar(e["launch"], e["composed"], dtype, f"densebn-eval/{slug(name)} relu={int(relu)}")


@pytest.mark.parametrize("name", B.DENSEBN_EVAL_AND_F16, ids=[slug(n) for n in B.DENSEBN_EVAL_AND_F16])
def test_densebn_branch_float16_forward(name):
    dtype = torch.float16
    case = B.densebn(name, dtype)
    args = TN.on_device(case["layout"], dtype, seed=3)
    with torch.no_grad():
        TN.compare(f"densebn-f16/{slug(name)}", *args, dtype, True, grads=False)
