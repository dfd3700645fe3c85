"""csrc/bertnorm.hip on the device: the launch (`route="launch"`) against the float64 restatement of
tests/_bertnorm_ref.py, with the composed torch route in the same input type as the yardstick.  With e_f the launch's
error and e_c the composed route's, both against float64 on the same (already rounded) inputs, and u one unit of the
delivered type (2^-23 float32, 2^-8 bfloat16, 2^-11 float16):

    y              max_ij |err_ij| / A_ij    A_ij = |gamma_j| (|s_ij| + |mean_i|) rstd_i + |beta_j|     e_f <= 2 max(e_c, u)
    dx, dres,      max |err| / max |float64 gradient|                                                   e_f <= 2 max(e_c, u)
    dgamma, dbeta  (a float64 gradient that is exactly zero -- dx and dgamma at hidden = 1, dx under a zero gamma -- has
                   no max norm: there the scale is max |g| max |gamma|)

A is the running-error scale of the cancellation in s - mean.  The factor two: the routes add the same terms in another
order; the floor u: a composed route that lands exactly must not fail the launch.  Every case prints both errors (run
with -s to see them); DESIGN.md section 21 quotes the worst."""
import pytest
import torch

import _bertnorm_ref as R
from tadmm import _cabi, ops
from tadmm import functional as HF
from tadmm import bert_layers as BL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UNIT = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
HMAX = ops.bertnorm_hmax()
BWD_GRID = ops.bertnorm_workspace_bytes(10 ** 6, 64) // (2 * 64 * 4)       # workgroups of the backward's row launch
# more rows than the backward's grid owns in one trip of four: every wave adds several rows into its dgamma registers
MANY_ROWS = 2 * 4 * BWD_GRID + 7

SHAPES = [(1, 1), (3, 5), (7, 63), (4, 64), (5, 65), (130, 312), (17, 768), (33, 1000), (9, 1024), (2, HMAX),
          (MANY_ROWS, 64)]
LAYOUTS = ("plain", "slice", "odd")
# (with a residual, dropout probability, parameters in the type of x)
VARIANTS = [(True, 0.0, False), (True, 0.1, True), (False, 0.1, False), (False, 0.0, True)]
GRADS = ("dx", "dres", "dgamma", "dbeta")


def place(t, layout, dtype):
    """A CPU float32 tensor (rows, hidden) on the device in `dtype`: as it is, or starting one element into its allocation."""
    t = t.to(dtype)
    if layout != "odd":
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=dtype, device=DEV)
    buf[1:].copy_(t.reshape(-1))
    v = buf[1:].view(t.shape)
    assert (v.data_ptr() // v.element_size()) % 2 == 1
    return v


def make_inputs(rows, hidden, layout, dtype, seed, kind="normal"):
    """x, res (rows, hidden) on the device: two tensors, column slices of one wider tensor (row stride > hidden), or
    tensors that start one element into their allocation; gamma, beta, the upstream gradient g (float32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    x, res = torch.randn(rows, hidden, generator=g), torch.randn(rows, hidden, generator=g)
    gamma, beta = 1 + 0.5 * torch.randn(hidden, generator=g), torch.randn(hidden, generator=g)
    up = torch.randn(rows, hidden, generator=g)
    if kind == "constant":
        x, res = torch.full((rows, hidden), 2.5), torch.full((rows, hidden), -0.75)
    elif kind == "offset":                             # mean / std around 1e5
        x, res = 400 + 0.01 * x, 600 + 0.01 * res
    elif kind == "spike":
        x[:, hidden // 3] = 3.0e4
    elif kind == "zero_gamma":
        gamma = torch.zeros(hidden)
    if layout == "slice":
        # hidden a multiple of 8: slices that keep 16-byte alignment (the vector path under a row stride > hidden);
        # otherwise slices at odd offsets under an odd row stride
        a, b = (8, 8) if hidden % 8 == 0 else (3, 2)
        wide = torch.cat([x, torch.zeros(rows, a), res, torch.zeros(rows, b)], dim=1).to(dtype).to(DEV)
        x, res = wide[:, :hidden], wide[:, hidden + a:2 * hidden + a]
        assert x.stride(0) == 2 * hidden + a + b and res.stride(0) == 2 * hidden + a + b
    else:
        x, res = place(x, layout, dtype), place(res, layout, dtype)
    return x, res, gamma, beta, up


def y_err(got, ref):
    got = got.detach().to("cpu", torch.float64)
    return float(((got - ref["y"]).abs() / ref["A"].clamp_min(1e-300)).max())


def grad_err(got, want, natural):
    scale = float(want.abs().max()) or natural
    err = float((got.detach().to("cpu", torch.float64).reshape(want.shape) - want).abs().max())
    if scale == 0.0:                                   # a zero gamma under the rule above: only exact zeros will do
        return 0.0 if err == 0.0 else float("inf")
    return err / scale


def bar(e_f, e_c, dtype, what):
    print(f"    {what:<40s} launch {e_f:.3e}   composed {e_c:.3e}   unit {UNIT[dtype]:.3e}")
    assert e_f <= 2.0 * max(e_c, UNIT[dtype]), (what, e_f, e_c)
    return e_c


def run_both(x, res, gamma, beta, up, p, keep, grads=True):
    """{route: (y, [dx, dres, dgamma, dbeta])} with None for what does not exist; leaves keep the strides of x and res."""
    out = {}
    for route in ("launch", "composed"):
        leaves = [None if t is None else t.detach().requires_grad_(grads) for t in (x, res, gamma, beta)]
        assert leaves[0].stride() == x.stride() and leaves[0].data_ptr() == x.data_ptr()
        y = HF.residual_layer_norm(*leaves, dropout_p=p, training=p > 0, keep=keep, route=route)
        assert y.shape == x.shape and y.dtype == x.dtype and (route == "composed" or y.is_contiguous())
        got = [None] * 4
        if grads:
            have = [i for i, t in enumerate(leaves) if t is not None]
            for i, gr in zip(have, torch.autograd.grad(y, [leaves[i] for i in have], up)):
                got[i] = gr
        out[route] = (y, got)
    return out


def compare(tag, x, res, gamma, beta, up, p, keep, dtype, grads=True):
    ref = R.restate(x, res, gamma, beta, p=p, keep=keep, g=up if grads else None)
    both = run_both(x, res, gamma, beta, up, p, keep, grads)
    e_c = {"y": bar(y_err(both["launch"][0], ref), y_err(both["composed"][0], ref), dtype, f"{tag} y")}
    if grads:
        natural = float(up.abs().max()) * float(gamma.abs().max())
        for i, name in enumerate(GRADS):
            if both["launch"][1][i] is None:
                assert name == "dres" and res is None
                continue
            assert both["launch"][1][i].dtype == (x, res, gamma, beta)[i].dtype
            e_c[name] = bar(grad_err(both["launch"][1][i], ref[name], natural),
                            grad_err(both["composed"][1][i], ref[name], natural), dtype, f"{tag} {name}")
        dx, dres = both["launch"][1][:2]
        if dres is not None:                           # never one tensor for two inputs
            assert dx.untyped_storage().data_ptr() != dres.untyped_storage().data_ptr()
            if p == 0.0:
                assert torch.equal(dx, dres)
    return e_c


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{r}x{h}" for r, h in SHAPES])
def test_forward_and_backward_against_float64(shape, dtype, layout):
    rows, hidden = shape
    x, res, gamma, beta, up = make_inputs(rows, hidden, layout, dtype, seed=rows * 7 + hidden)
    if layout != "plain":                              # read in place: no copy is made of such views
        for t in (x, res):
            assert ops._bertnorm_rows(t, "t", "t", tuple(t.shape), dtype)[0].data_ptr() == t.data_ptr()
    gk = torch.Generator(device=DEV).manual_seed(hidden)
    up = up.to(dtype).to(DEV)
    for with_res, p, same_type in VARIANTS:
        pdt = dtype if same_type else torch.float32
        keep = HF.residual_keep_mask((rows, hidden), p, DEV, generator=gk) if p > 0 else None
        print(f"  {rows}x{hidden} {dtype} {layout} res={with_res} p={p} params={pdt}")
        compare("", x, res if with_res else None, gamma.to(pdt).to(DEV), beta.to(pdt).to(DEV), up, p, keep, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["constant", "offset", "spike", "zero_gamma"])
def test_hard_rows(kind, dtype):
    """Rows that are hard for the row statistics.  The upstream gradient is positive here: with one huge element in
    column c every row has xhat_ic = sqrt(hidden - 1), so dgamma_c = sqrt(hidden - 1) sum_i g_ic is the largest entry of
    dgamma and sets the scale of its error measure.  Under a gradient of random sign that sum cancels (condition
    sum |g| / |sum g|, unbounded over a handful of rows) and multiplies the half unit that a float32 rstd carries on
    either route, so which route lands inside twice the other's error is a coin toss (measured so, (9, 312) float32:
    launch 5.0e-7, composed 2.2e-7, both from per-term errors of one unit).  A positive gradient has condition 1 and
    leaves the case to what it is about."""
    for rows, hidden in ((9, 312), (5, 65), (6, 1024)):
        x, res, gamma, beta, up = make_inputs(rows, hidden, "plain", dtype, seed=31 + hidden, kind=kind)
        print(f"  {kind} {rows}x{hidden} {dtype}")
        e_c = compare(kind, x, res, gamma.to(DEV), beta.to(DEV), up.abs().to(dtype).to(DEV), 0.0, None, dtype)
        if kind == "offset" and dtype == torch.float32:
            # the yardstick itself is sound on these rows (checked on the CPU in float32 for seeds 0 .. 3: 0.3 - 0.6 u)
            assert e_c["y"] <= 2.0 * UNIT[dtype], e_c


def test_float16_is_forward_only():
    dtype = torch.float16
    for rows, hidden, layout in ((130, 312, "plain"), (5, 65, "odd"), (17, 768, "slice")):
        x, res, gamma, beta, up = make_inputs(rows, hidden, layout, dtype, seed=3)
        for pdt in (torch.float32, dtype):
            compare("f16", x, res, gamma.to(pdt).to(DEV), beta.to(pdt).to(DEV), None, 0.0, None, dtype, grads=False)
    gamma, beta = gamma.to(DEV), beta.to(DEV)
    y, stats = ops.bertnorm_fwd(x, res, gamma, beta, need_stats=True)
    with pytest.raises(_cabi.TadmmError, match="forward only"):
        ops.bertnorm_bwd(x, res, gamma, stats, y)
    with pytest.raises(_cabi.TadmmError, match="float16 with gradients"):
        HF.residual_layer_norm(x.detach().requires_grad_(), res, gamma, beta, route="launch")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_two_backward_runs_are_bit_identical(dtype):
    rows, hidden = MANY_ROWS, 312
    x, res, gamma, beta, up = make_inputs(rows, hidden, "plain", dtype, seed=5)
    gamma, beta, up = gamma.to(DEV), beta.to(DEV), up.to(dtype).to(DEV)
    keep = HF.residual_keep_mask((rows, hidden), 0.1, DEV)
    other = make_inputs(33, 1000, "plain", dtype, seed=6)
    runs = []
    for n in range(2):
        leaves = [t.detach().requires_grad_() for t in (x, res, gamma, beta)]
        y = HF.residual_layer_norm(*leaves, dropout_p=0.1, training=True, keep=keep, route="launch")
        runs.append((y,) + torch.autograd.grad(y, leaves, up))
        if n == 0:                                     # a call of another shape in between
            o = [t.to(DEV).requires_grad_() if t.device.type == "cpu" else t.detach().requires_grad_() for t in other[:4]]
            HF.residual_layer_norm(*o, route="launch").sum().backward()
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert runs[0][1].untyped_storage().data_ptr() != runs[0][2].untyped_storage().data_ptr()


def test_recorded_reference_through_the_modules(golden_dir):
    """G19 (the reference's own BertLayerNorm, TTBertSelfOutput and BertOutput on the CPU, float32) through the modules
    with the projection replaced by the `weights=` hook: 1e-5 of the largest magnitude, float32 against a float32 run in
    another order."""
    class Hook:
        def __init__(self, x):
            self.x = x

        def output_transform(self, hidden_states, layer_id):
            return self.x

        def ffn_output_transform(self, hidden_states, layer_id):
            return self.x

    for meta in R.golden_index(golden_dir):
        d = {key: t.to(DEV) for key, t in R.recorded(golden_dir, meta).items()}
        shape = (meta["B"], meta["S"], meta["hidden"])
        x = d["x"].view(shape).requires_grad_()
        if meta["module"] == "BertLayerNorm":
            mod = BL.BertLayerNorm(meta["hidden"]).to(DEV).eval()
            norm, leaves = mod, [x]
        else:
            cls = BL.BertSelfOutput if meta["module"] == "TTBertSelfOutput" else BL.BertOutput
            mod = (cls(meta["hidden"], 0.1) if cls is BL.BertSelfOutput else cls(4 * meta["hidden"], meta["hidden"], 0.1))
            mod = mod.to(DEV).eval()
            norm = mod.LayerNorm
            leaves = [x, d["res"].view(shape).requires_grad_()]
        mod.route = "launch"
        with torch.no_grad():
            norm.weight.copy_(d["weight"])
            norm.bias.copy_(d["bias"])
        y = mod(x) if len(leaves) == 1 else mod(torch.zeros(shape, device=DEV), leaves[1], weights=Hook(x))
        grads = torch.autograd.grad(y, leaves + [norm.weight, norm.bias], d["g"].view(shape))
        names = ["dx"] + (["dres"] if len(leaves) == 2 else []) + ["dweight", "dbias"]
        for got, key in zip((y,) + grads, ["y"] + names):
            want = d[key].view(got.shape)
            assert float((got.detach() - want).abs().max()) <= 1e-5 * float(want.abs().max()), (meta, key)


def test_module_dropout_follows_the_seed_and_wide_rows_take_the_composed_route():
    torch.manual_seed(0)
    mod = BL.BertSelfOutput(96, 0.1).to(DEV).train()
    mod.route = "launch"
    x, res = torch.randn(2, 37, 96, device=DEV), torch.randn(2, 37, 96, device=DEV)
    outs = []
    for seed in (11, 11, 12):
        torch.manual_seed(seed)
        outs.append(mod(x, res))
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    wide = torch.randn(3, HMAX + 8, device=DEV)
    w, b = torch.ones(HMAX + 8, device=DEV), torch.zeros(HMAX + 8, device=DEV)
    assert torch.equal(HF.residual_layer_norm(wide, None, w, b), HF.residual_layer_norm_composed(wide, None, w, b))
    with pytest.raises(_cabi.TadmmError):
        HF.residual_layer_norm(wide, None, w, b, route="launch")
    t = torch.randn(4, 6, 8, 40, device=DEV)[:, ::2]                # leading dimensions that do not flatten: copied
    w, b = torch.rand(40, device=DEV), torch.rand(40, device=DEV)
    assert torch.allclose(HF.residual_layer_norm(t, t, w, b, route="launch"),
                          HF.residual_layer_norm_composed(t, t, w, b), atol=1e-5)


def test_bert_layer_against_float64():
    """A whole BertLayer at BERT-base sizes with the reference's TT shapes, float32, every route forced to the launch,
    against the same module in float64 on the CPU; the composed routes are the yardstick under the same bar, in the max
    norm: output, attention scores and every parameter gradient."""
    torch.manual_seed(4)
    B, S = 2, 16
    layer = BL.BertLayer(768, 12, 3072, linear=BL.reference_tt_linear, layer_id=0).eval()
    with torch.no_grad():
        for m in (layer.attention.output.LayerNorm, layer.output.LayerNorm):
            m.weight.uniform_(0.5, 1.5)
            m.bias.uniform_(-0.5, 0.5)
    x = torch.randn(B, S, 768)
    mask = torch.zeros(B, 1, 1, S)
    mask[1, 0, 0, 11:] = -10000.0
    up = torch.randn(B, S, 768)
    names = [n for n, _ in layer.named_parameters()]

    def run(mod, x, mask, up):
        out, att = mod(x, mask)
        grads = torch.autograd.grad(out, list(mod.parameters()), up)
        return [out.detach(), att.detach()] + [g.detach() for g in grads]

    ref = run(layer.double(), x.double(), mask.double(), up.double())
    layer = layer.float().to(DEV)
    got = {}
    for route in ("launch", "composed"):
        got[route] = run(layer.set_route(route), x.to(DEV), mask.to(DEV), up.to(DEV))
    worst = 0.0
    for i, what in enumerate(["output", "scores"] + names):
        scale = float(ref[i].abs().max())
        e_f, e_c = (float((got[r][i].to("cpu", torch.float64) - ref[i]).abs().max()) / scale for r in ("launch", "composed"))
        bar(e_f, e_c, torch.float32, what)
        worst = max(worst, e_f)
    print(f"    worst launch error of the layer {worst:.3e}")
