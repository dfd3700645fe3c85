"""csrc/densebn.hip on the device: the launch (`route="launch"`) against the float64 restatement of
tests/_densenet_ref.py, with the composed torch route (torch.cat + F.batch_norm + relu) in the same input type as the
yardstick -- the bar of tests/test_gpu_bnact.py.  With e_f the launch's error and e_c the composed route's, both against
float64 on the same (already rounded) inputs and both max |err| / max |float64 value|, and u one unit of the delivered type
(2^-23 float32, 2^-8 bfloat16, 2^-11 float16):

    e_f <= 2 max(e_c, u)     for y, every segment's gradient, dgamma, dbeta, running_mean and running_var.

The float64 gradients take the ReLU mask of the route being judged from its own stored y: the rounding of y is judged
once, in the forward, and no element is left out.  A float64 value that is exactly zero everywhere (y == 0, dx under a
zero gamma) has no max norm: there the scale is max |g| max(1, |gamma|), and y must be exactly zero.

Every case prints both errors (run with -s to see them)."""
import pytest
import torch

import _densenet_ref as D
from tadmm import _cabi, ops
from tadmm import functional as HF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UNIT = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}

# name -> (channels of the segments, N, H, W, index of the segment placed one element past a 16-byte boundary)
LAYOUTS = {
    "element-5+3+3-n2-5x5": ((5, 3, 3), 2, 5, 5, None),            # H W is no whole number of 16-byte units
    "wide-8+4+4-n3-8x8": ((8, 4, 4), 3, 8, 8, None),               # the 16-byte path
    "trips-5+3+3-n4-24x24": ((5, 3, 3), 4, 24, 24, None),          # M = 2304: three float32 trips, a split per trip,
                                                                   # and splits that cross image boundaries (H W = 576)
    "odd-8+4+4-n3-8x8": ((8, 4, 4), 3, 8, 8, 1),                   # one misaligned base sends every access to elements
    "65x1-n2-4x4": ((1,) * 65, 2, 4, 4, None),                     # the 64-layer block of DenseNet-264 at its norm5
}


def place(t, dtype, odd=False):
    """A CPU float32 tensor on the device in `dtype`: as it is, or starting one element into its allocation."""
    t = t.to(dtype)
    if not odd:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=dtype, device=DEV)
    buf[1:].copy_(t.reshape(-1))
    v = buf[1:].view(t.shape)
    assert (v.data_ptr() // v.element_size()) % 2 == 1 and v.is_contiguous()
    return v


def make_inputs(chans, n, h, w, seed, kind="normal"):
    """The segments, gamma, beta, the upstream gradient and running statistics (float32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    c = sum(chans)
    segs = [0.5 + 2 * torch.randn(n, ck, h, w, generator=g) for ck in chans]
    gamma, beta = 1 + 0.5 * torch.randn(c, generator=g), torch.randn(c, generator=g)
    up = torch.randn(n, c, h, w, generator=g)
    rm, rv = torch.randn(c, generator=g), 0.5 + torch.rand(c, generator=g)
    if kind == "constant":                             # the variance is 0
        segs = [torch.full_like(s, 2.5) for s in segs]
    elif kind == "offset":                             # mean / std around 1e5: the shifted sums
        segs = [1000 + 0.01 * s for s in segs]
    elif kind == "negative":                           # every pre-activation below zero: y == 0, the gradients exact zeros
        beta = -100 - beta.abs()
    elif kind == "zero_gamma":
        gamma = torch.zeros(c)
    return segs, gamma, beta, up, rm, rv


def max_err(got, want, natural=None):
    want = want.detach()
    scale = float(want.abs().max()) or (natural or 0.0)
    err = float((got.detach().to("cpu", torch.float64).reshape(want.shape) - want).abs().max())
    if scale == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / scale


def bar(e_f, e_c, dtype, what):
    print(f"    {what:<52s} launch {e_f:.3e}   composed {e_c:.3e}   unit {UNIT[dtype]:.3e}")
    assert e_f <= 2.0 * max(e_c, UNIT[dtype]), (what, e_f, e_c)
    return e_f


def run_route(route, segs, gamma, beta, up, rm, rv, relu, grads, momentum=0.1, eps=1e-5, plain=False):
    """One training call on fresh leaves over the same storage: y, the updated running statistics, the gradients
    [dx_0 .. dx_{k-1}, dgamma, dbeta]."""
    leaves = [t.detach().requires_grad_(grads) for t in list(segs) + [gamma, beta]]
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(leaves, segs))
    rm_, rv_, nbt = rm.clone(), rv.clone(), torch.tensor(5, device=DEV)
    feats = leaves[0] if plain else HF.DenseFeatures(leaves[:-2])
    y = HF.dense_batch_norm_act(feats, rm_, rv_, leaves[-2], leaves[-1], training=True, momentum=momentum, eps=eps,
                                relu=relu, num_batches_tracked=nbt, route=route)
    c = sum(s.shape[1] for s in segs)
    assert y.shape == (segs[0].shape[0], c) + segs[0].shape[2:] and y.dtype == segs[0].dtype and int(nbt) == 6
    assert y.is_contiguous()
    got = list(torch.autograd.grad(y, leaves, up)) if grads else [None] * len(leaves)
    if grads and route == "launch":
        assert all(t.is_contiguous() and t.shape == s.shape and t.dtype == s.dtype for t, s in zip(got, leaves))
    return y.detach(), rm_, rv_, got


def compare(tag, segs, gamma, beta, up, rm, rv, dtype, relu, grads=True, momentum=0.1, eps=1e-5, plain=False):
    """Both routes against float64 under the rule of the module docstring; returns the launch's errors."""
    n, _, h, w = segs[0].shape
    ref = D.pre_act(segs, gamma, beta, relu, eps)
    ref_rm, ref_rv = D.R.running(rm, rv, ref["mean"], ref["var"], n * h * w, momentum)
    natural = float(up.abs().max()) * max(1.0, float(gamma.abs().max()))
    err = {}
    for route in ("launch", "composed"):
        y, rm_, rv_, got = run_route(route, segs, gamma, beta, up, rm, rv, relu, grads, momentum, eps, plain)
        e = {"y": max_err(y, ref["y"]), "running_mean": max_err(rm_, ref_rm), "running_var": max_err(rv_, ref_rv)}
        if grads:
            want = D.pre_act_grads(segs, gamma, beta, up, (y > 0) if relu else None, eps)
            for k in range(len(segs)):
                e[f"dx{k}"] = max_err(got[k], want["dx"][k], natural)
            e["dgamma"] = max_err(got[-2], want["dgamma"], natural)
            e["dbeta"] = max_err(got[-1], want["dbeta"], natural)
        err[route] = e
    return {k: bar(err["launch"][k], err["composed"][k], dtype, f"{tag} {k}") for k in err["launch"]}


def on_device(case, dtype, seed, kind="normal"):
    chans, n, h, w, odd = case
    segs, gamma, beta, up, rm, rv = make_inputs(chans, n, h, w, seed, kind)
    segs = [place(s, dtype, odd == k) for k, s in enumerate(segs)]
    return segs, gamma.to(DEV), beta.to(DEV), up.to(dtype).to(DEV), rm.to(DEV), rv.to(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_segment_layouts_against_float64(name, dtype):
    args = on_device(LAYOUTS[name], dtype, seed=len(name))
    for relu in (True, False):
        compare(f"{name} relu={int(relu)}", *args, dtype, relu)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_a_plain_tensor_is_one_segment(dtype):
    for shape, odd in (((2, 6, 5, 5), None), ((3, 8, 8, 8), None), ((3, 8, 8, 8), 0)):
        args = on_device(((shape[1],), shape[0], shape[2], shape[3], odd), dtype, seed=shape[1])
        compare(f"plain {shape} odd={odd}", *args, dtype, True, plain=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_shared_segments_of_three_chained_layers(dtype):
    """Three layers on one DenseFeatures, each with its own gamma, beta and eps; a layer's new segment is a copy of the
    first channels of its y (exact in every type, so nothing but the pre-activations is judged).  The first segment is
    consumed three times: its summed gradient, every layer's dgamma and dbeta and the last y against the float64 of the
    same chain; a segment keeps one stats tensor for the life of the holder."""
    n, h, w, c0, grow = 3, 8, 8, 8, 4
    g = torch.Generator().manual_seed(21)
    x0 = place(0.5 + 2 * torch.randn(n, c0, h, w, generator=g), dtype)
    widths = [c0, c0 + grow, c0 + 2 * grow]
    params = [((1 + 0.5 * torch.randn(c, generator=g)).to(DEV), torch.randn(c, generator=g).to(DEV)) for c in widths]
    epss = [1e-5, 1e-3, 1e-1]
    up = torch.randn(n, widths[2], h, w, generator=g).to(dtype).to(DEV)

    def chain(route):
        x = x0.detach().requires_grad_()
        leaves = [x] + [t.detach().requires_grad_() for pair in params for t in pair]
        feats = HF.DenseFeatures(x)
        ys, kept = [], []
        for i in range(3):
            c = widths[i]
            y = HF.dense_batch_norm_act(feats, torch.zeros(c, device=DEV), torch.ones(c, device=DEV), leaves[1 + 2 * i],
                                        leaves[2 + 2 * i], training=True, eps=epss[i], route=route)
            ys.append(y)
            if route == "launch":
                kept.append(list(feats._stats))
            if i < 2:
                feats.append(y[:, :grow].contiguous())
        if route == "launch":                           # the same objects after the second and the third layer
            assert all(s is not None for s in kept[2]) and kept[0][0] is kept[1][0] is kept[2][0]
            assert kept[1][1] is kept[2][1] and kept[0][0].dtype == torch.float64 and kept[0][0].shape == (c0, 2)
        else:
            assert feats._stats == [None] * 3
        return ys, torch.autograd.grad(ys[2], leaves, up)

    def chain64(masks):
        x = D.f64(x0).requires_grad_()
        leaves = [x] + [D.f64(t).requires_grad_() for pair in params for t in pair]
        feats = [x]
        for i in range(3):
            y = D.pre_act_graph(feats, leaves[1 + 2 * i], leaves[2 + 2 * i], masks[i], epss[i])
            if i < 2:
                feats.append(y[:, :grow])
        return y, torch.autograd.grad(y, leaves, D.f64(up))

    err = {}
    for route in ("launch", "composed"):
        ys, grads = chain(route)
        want_y, want = chain64([y > 0 for y in ys])
        natural = float(up.abs().max())
        e = {"y": max_err(ys[2], want_y), "dx0 (three consumers)": max_err(grads[0], want[0], natural)}
        for i in range(3):
            e[f"dgamma{i}"] = max_err(grads[1 + 2 * i], want[1 + 2 * i], natural)
            e[f"dbeta{i}"] = max_err(grads[2 + 2 * i], want[2 + 2 * i], natural)
        err[route] = e
    for k in err["launch"]:
        bar(err["launch"][k], err["composed"][k], dtype, f"chain {k}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["constant", "offset", "negative", "zero_gamma"])
def test_hard_channels(kind, dtype):
    for name in ("element-5+3+3-n2-5x5", "wide-8+4+4-n3-8x8", "trips-5+3+3-n4-24x24"):
        args = on_device(LAYOUTS[name], dtype, seed=31, kind=kind)
        e = compare(f"{kind} {name}", *args, dtype, True)
        if kind == "negative":                         # y == 0: exact zeros, not small numbers
            assert all(v == 0.0 for k, v in e.items() if k.startswith("d"))
            y, _, _, got = run_route("launch", *args, True, True)
            assert int(y.ne(0).sum()) == 0 and all(int(t.ne(0).sum()) == 0 for t in got)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_eval_mode_is_the_folded_formula_and_writes_no_statistics(dtype):
    for name, case in LAYOUTS.items():
        segs, gamma, beta, up, rm, rv = on_device(case, dtype, seed=7)
        for relu in (True, False):
            want = D.pre_act_eval(segs, rm, rv, gamma, beta, relu)
            e = {}
            for route in ("launch", "composed"):
                rm_, rv_, nbt = rm.clone(), rv.clone(), torch.tensor(5, device=DEV)
                feats = HF.DenseFeatures(segs)
                with torch.no_grad():
                    y = HF.dense_batch_norm_act(feats, rm_, rv_, gamma, beta, training=False, relu=relu,
                                                num_batches_tracked=nbt, route=route)
                assert torch.equal(rm_, rm) and torch.equal(rv_, rv) and int(nbt) == 5     # eval touches nothing
                assert feats._stats == [None] * len(segs)                                   # and computes no statistics
                e[route] = max_err(y, want)
            bar(e["launch"], e["composed"], dtype, f"eval {name} relu={int(relu)}")


def test_float16_is_forward_only():
    dtype = torch.float16
    for name in ("element-5+3+3-n2-5x5", "wide-8+4+4-n3-8x8", "odd-8+4+4-n3-8x8"):
        args = on_device(LAYOUTS[name], dtype, seed=3)
        with torch.no_grad():
            compare(f"f16 {name}", *args, dtype, True, grads=False)
    segs, gamma, beta, up, rm, rv = args
    stats = [ops.densebn_stats(s) for s in segs]
    y = ops.densebn_fwd(segs, stats, gamma, beta, rm.clone(), rv.clone(), training=True)
    with pytest.raises(_cabi.TadmmError, match="forward only"):
        ops.densebn_bwd(up, y, segs, stats, gamma)
    with pytest.raises(_cabi.TadmmError, match="float16 with gradients"):
        HF.dense_batch_norm_act([segs[0].requires_grad_()] + segs[1:], rm, rv, gamma, beta, training=True, route="launch")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_bookkeeping_and_reproducibility(dtype):
    segs, gamma, beta, up, rm, rv = on_device(LAYOUTS["trips-5+3+3-n4-24x24"], dtype, seed=5)
    other = on_device(LAYOUTS["element-5+3+3-n2-5x5"], dtype, seed=6)
    runs = []
    nbt = torch.tensor(0, device=DEV)
    for i in range(2):
        leaves = [t.detach().requires_grad_() for t in segs + [gamma, beta]]
        rm_, rv_ = rm.clone(), rv.clone()
        y = HF.dense_batch_norm_act(leaves[:3], rm_, rv_, leaves[3], leaves[4], training=True, num_batches_tracked=nbt,
                                    route="launch")
        assert int(nbt) == i + 1                        # the batch counter counts
        runs.append((y, rm_, rv_) + torch.autograd.grad(y, leaves, up))
        if i == 0:                                      # a call of another shape in between
            o = [t.detach().requires_grad_() for t in other[0]]
            HF.dense_batch_norm_act(o, other[4].clone(), other[5].clone(), other[1], other[2], training=True,
                                    route="launch").sum().backward()
    for a, b in zip(*runs):
        assert torch.equal(a, b)                        # two runs are bit-identical
    with torch.no_grad():
        HF.dense_batch_norm_act(segs, rm, rv, gamma, beta, training=False, num_batches_tracked=nbt, route="launch")
    assert int(nbt) == 2
    # a segment without requires_grad gets no gradient and no dx is written for it; the others are unchanged to the bit
    leaves = [segs[0].detach().requires_grad_(), segs[1].detach(), segs[2].detach().requires_grad_()]
    y = HF.dense_batch_norm_act(leaves, rm.clone(), rv.clone(), gamma, beta, training=True, route="launch")
    d0, d2 = torch.autograd.grad(y, [leaves[0], leaves[2]], up)
    assert torch.equal(d0, runs[0][3]) and torch.equal(d2, runs[0][5]) and torch.equal(y, runs[0][0])
    stats = [ops.densebn_stats(s) for s in segs]
    dxs, dgamma, dbeta = ops.densebn_bwd(up, y.detach(), segs, stats, gamma, need_dx=(True, False, True))
    assert dxs[1] is None and torch.equal(dxs[0], d0) and torch.equal(dxs[2], d2)
    assert torch.equal(dgamma, runs[0][6]) and torch.equal(dbeta, runs[0][7])
    dxs, dgamma, dbeta = ops.densebn_bwd(up, y.detach(), segs, stats, gamma, need_dx=(False,) * 3, need_dgamma=False,
                                         need_dbeta=False)
    assert dxs == [None] * 3 and dgamma is None and dbeta is None
    dxs, dgamma, dbeta = ops.densebn_bwd(up, y.detach(), segs, stats, gamma, need_dx=(False, True, False), need_dgamma=False)
    assert dgamma is None and torch.equal(dxs[1], runs[0][4]) and torch.equal(dbeta, runs[0][7])
    # the statistics of a segment: float64 (C_k, 2) = (mean, biased variance), the same bits on every call
    ref = D.pre_act(segs, gamma, beta)
    got = torch.cat(stats, 0)
    assert got.dtype == torch.float64 and torch.equal(got, torch.cat([ops.densebn_stats(s) for s in segs], 0))
    assert max_err(got[:, 0], ref["mean"]) <= 1e-13 and max_err(got[:, 1], ref["var"]) <= 1e-12
    # the running statistics are torch's, with the module's momentum
    for momentum in (0.1, 0.3):
        compare(f"momentum={momentum}", segs, gamma, beta, up, rm, rv, dtype, True, grads=False, momentum=momentum)
    # what the launch does not take raises under route="launch" before anything runs
    cl = [s.contiguous(memory_format=torch.channels_last) for s in segs]
    with pytest.raises(_cabi.TadmmError, match="NCHW contiguous"):
        HF.dense_batch_norm_act(cl, rm.clone(), rv.clone(), gamma, beta, training=True, route="launch")
    with pytest.raises(_cabi.TadmmError, match="momentum=None"):
        HF.dense_batch_norm_act(segs, rm.clone(), rv.clone(), gamma, beta, training=True, momentum=None, route="launch")
    with pytest.raises(_cabi.TadmmError, match="mixed types"):
        HF.dense_batch_norm_act([segs[0], segs[1].to(torch.float16)] + segs[2:], rm.clone(), rv.clone(), gamma, beta,
                                training=True, route="launch")
    with pytest.raises(_cabi.TadmmError, match="eval mode with gradients"):
        HF.dense_batch_norm_act([segs[0].detach().requires_grad_()] + segs[1:], rm, rv, gamma, beta, training=False,
                                route="launch")
