"""csrc/prenorm.hip on the device: the launch (`route="launch"`) against the float64 restatement of tests/_vit_ref.py,
with the composed torch route in the same input type as the yardstick -- the rule of tests/test_gpu_bertnorm.py.  With
e_f the launch's error and e_c the composed route's, both against float64 on the same (already rounded) inputs, and u
one unit of the delivered type (2^-23 float32, 2^-8 bfloat16, 2^-11 float16):

    s              max_ij |err_ij| / (|x_ij| + |scale_i b_ij keep_ij / (1 - p)|)                        e_f <= 2 max(e_c, u)
    y              max_ij |err_ij| / A_ij    A_ij = |gamma_j| (|s_ij| + |mean_i|) rstd_i + |beta_j|     e_f <= 2 max(e_c, u)
                   against the float64 LayerNorm of that route's own delivered s: the rounding of s is judged once, above
    dx, db,        max |err| / max |float64 gradient|                                                   e_f <= 2 max(e_c, u)
    dgamma, dbeta  (a float64 gradient that is exactly zero -- db of a dropped batch, dgamma without g_y, dx under a zero
                   gamma without g_s -- has no max norm: there the scale is max |g| max(1, |gamma|))

Every case prints both errors (run with -s to see them); DESIGN.md section 23 quotes the worst."""
import pytest
import torch

import _vit_ref as R
from tadmm import _cabi, ops
from tadmm import functional as HF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UNIT = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
HMAX = ops.bertnorm_hmax()
BWD_GRID = ops.prenorm_workspace_bytes(10 ** 6, 64) // (2 * 64 * 4)        # workgroups of the backward's row launch
# more rows than the backward's grid owns in two trips of four: every wave adds several rows into its dgamma registers
MANY_ROWS = 2 * 4 * BWD_GRID + 7

SHAPES = [(1, 1), (3, 5), (7, 63), (4, 64), (5, 65), (2 * 197, 192), (17, 384), (33, 1000), (2, HMAX), (MANY_ROWS, 64)]
LAYOUTS = ("plain", "slice", "odd")
GRADS = ("dx", "db", "dgamma", "dbeta")
# (dropout p, DropPath p_path, which samples DropPath drops, parameters in the type of x, gradient into s, into y)
VARIANTS = [(0.0, 0.0, None, False, True, True), (0.1, 0.0, None, True, True, True), (0.0, 0.5, "one", False, True, True),
            (0.0, 0.5, "all", False, True, True), (0.1, 0.5, "one", True, True, True),
            (0.0, 0.0, None, False, True, False), (0.1, 0.0, None, False, False, True)]


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
    """x, b (rows, hidden) on the device: two tensors, column slices of one wider tensor (row stride > hidden; offsets
    that keep 16-byte alignment where hidden is a multiple of 8, odd ones otherwise), or tensors that start one element
    into their allocation; gamma, beta and the upstream gradients g_s, g_y (float32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    x, b = torch.randn(rows, hidden, generator=g), torch.randn(rows, hidden, generator=g)
    gamma, beta = 1 + 0.5 * torch.randn(hidden, generator=g), torch.randn(hidden, generator=g)
    g_s, g_y = torch.randn(rows, hidden, generator=g), torch.randn(rows, hidden, generator=g)
    if kind == "constant":
        x, b = torch.full((rows, hidden), 2.5), torch.full((rows, hidden), -0.75)
    elif kind == "offset":                             # mean / std around 1e5
        x, b = 400 + 0.01 * x, 600 + 0.01 * b
    elif kind == "spike":
        x[:, hidden // 3] = 3.0e4
    elif kind == "zero_gamma":
        gamma = torch.zeros(hidden)
    if layout == "slice":
        pa, pb = (8, 8) if hidden % 8 == 0 else (3, 2)
        wide = torch.cat([x, torch.zeros(rows, pa), b, torch.zeros(rows, pb)], dim=1).to(dtype).to(DEV)
        x, b = wide[:, :hidden], wide[:, hidden + pa:2 * hidden + pa]
        assert x.stride(0) == 2 * hidden + pa + pb and b.stride(0) == x.stride(0)
    else:
        x, b = place(x, layout, dtype), place(b, layout, dtype)
    return x, b, gamma, beta, g_s, g_y


def grad_err(got, want, natural):
    scale = float(want.abs().max()) or natural
    err = float((got.detach().to("cpu", torch.float64).reshape(want.shape) - want).abs().max())
    if scale == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / scale


def bar(e_f, e_c, dtype, what):
    print(f"    {what:<44s} launch {e_f:.3e}   composed {e_c:.3e}   unit {UNIT[dtype]:.3e}")
    assert e_f <= 2.0 * max(e_c, UNIT[dtype]), (what, e_f, e_c)
    return e_f


def samples(x, nper):
    """The (rows, C) tensor as `add_layer_norm` takes it: 2-D for one row per sample, else (B, nper, C); a view."""
    if nper == 1:
        return x
    v = x.view(x.shape[0] // nper, nper, x.shape[1])
    assert v.data_ptr() == x.data_ptr()
    return v


def run_both(x, b, gamma, beta, g_s, g_y, nper, p, keep, p_path, path_keep, grads=True):
    """{route: (s, y, [dx, db, dgamma, dbeta])}; the leaves keep the strides of x and b."""
    out = {}
    for route in ("launch", "composed"):
        leaves = [t.detach().requires_grad_(grads) for t in (samples(x, nper), samples(b, nper), gamma, beta)]
        assert leaves[0].data_ptr() == x.data_ptr() and leaves[1].data_ptr() == b.data_ptr()
        s, y = HF.add_layer_norm(*leaves, dropout_p=p, drop_path_p=p_path, training=p > 0 or p_path > 0,
                                 keep=None if keep is None else samples(keep, nper), path_keep=path_keep, route=route)
        assert s.shape == leaves[0].shape and y.shape == s.shape and s.dtype == x.dtype and y.dtype == x.dtype
        assert route == "composed" or (s.is_contiguous() and y.is_contiguous())
        got = [None] * 4
        if grads:
            outs, ups = zip(*[(o, samples(u, nper)) for o, u in ((s, g_s), (y, g_y)) if u is not None])
            got = list(torch.autograd.grad(outs, leaves, ups, allow_unused=True))
            for i in (2, 3):                           # without g_y the parameters see no gradient: zeros
                if got[i] is None:
                    assert g_y is None and route == "composed"
                    got[i] = torch.zeros_like(leaves[i])
        out[route] = (s.reshape(x.shape), y.reshape(x.shape), got)
    return out


def compare(tag, x, b, gamma, beta, g_s, g_y, dtype, nper=1, p=0.0, keep=None, p_path=0.0, path_keep=None, grads=True):
    """Both routes against float64 under the rule of the module docstring; returns the launch's errors."""
    s_ref, s_scale, factor = R.stream(x, b, p, keep, p_path, path_keep, nper)
    both = run_both(x, b, gamma, beta, g_s, g_y, nper, p, keep, p_path, path_keep, grads)
    e = {}
    err = {}
    for route in both:
        s, y, _ = both[route]
        ln = R.layer_norm(s, gamma, beta)              # of this route's own delivered s
        err[route] = (float(((R.f64(s) - s_ref).abs() / s_scale.clamp_min(1e-300)).max()),
                      float(((R.f64(y) - ln["y"]).abs() / ln["A"].clamp_min(1e-300)).max()))
    e["s"] = bar(err["launch"][0], err["composed"][0], dtype, f"{tag} s")
    e["y"] = bar(err["launch"][1], err["composed"][1], dtype, f"{tag} y")
    if grads:
        ref = R.tail_grads(s_ref, gamma, factor, g_y, g_s)
        natural = max(float(t.abs().max()) for t in (g_s, g_y) if t is not None) * max(1.0, float(gamma.abs().max()))
        for i, name in enumerate(GRADS):
            got = both["launch"][2][i]
            assert got.dtype == (x, b, gamma, beta)[i].dtype
            e[name] = bar(grad_err(got, ref[name], natural), grad_err(both["composed"][2][i], ref[name], natural), dtype,
                          f"{tag} {name}")
        dx, db = both["launch"][2][:2]                 # never one tensor for two inputs
        assert dx.untyped_storage().data_ptr() != db.untyped_storage().data_ptr()
        if p == 0.0 and p_path == 0.0:
            assert torch.equal(dx, db)
    if path_keep is not None and p_path > 0:           # a dropped sample: the stream passes untouched, bit for bit
        dead = (path_keep == 0).repeat_interleave(nper)
        s = both["launch"][0]
        assert dead.any()
        assert torch.equal(s[dead].view(BITS[dtype]), x[dead].contiguous().view(BITS[dtype]))
        if grads:
            db = both["launch"][2][1].reshape(x.shape)
            assert int(db[dead].contiguous().view(BITS[dtype]).ne(0).sum()) == 0
    return e


def structures(rows):
    """rows per sample: every row its own sample, one sample of all rows, and two samples of 197 tokens"""
    return sorted({1, rows} | ({197} if rows == 2 * 197 else set()))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{r}x{h}" for r, h in SHAPES])
def test_forward_and_backward_against_float64(shape, dtype, layout):
    rows, hidden = shape
    x, b, gamma, beta, g_s, g_y = make_inputs(rows, hidden, layout, dtype, seed=rows * 7 + hidden)
    if layout != "plain":                              # read in place: no copy is made of such views
        for t in (x, b):
            assert ops._bertnorm_rows(t, "t", "t", tuple(t.shape), dtype)[0].data_ptr() == t.data_ptr()
    gk = torch.Generator(device=DEV).manual_seed(hidden)
    g_s, g_y = g_s.to(dtype).to(DEV), g_y.to(dtype).to(DEV)
    for nper in structures(rows):
        B = rows // nper
        for p, p_path, dropped, same_type, with_gs, with_gy in VARIANTS:
            pdt = dtype if same_type else torch.float32
            keep = HF.residual_keep_mask((rows, hidden), p, DEV, generator=gk) if p > 0 else None
            path_keep = None
            if p_path > 0:
                path_keep = torch.zeros(B, dtype=torch.uint8, device=DEV)
                if dropped == "one" and B > 1:         # one sample of two dropped (a single sample can only be dropped)
                    path_keep[1::2] = 1
            tag = f"N={nper} p={p} path={p_path}/{dropped} params={str(pdt)[6:]} gs={int(with_gs)} gy={int(with_gy)}"
            compare(tag, x, b, gamma.to(pdt).to(DEV), beta.to(pdt).to(DEV), g_s if with_gs else None,
                    g_y if with_gy else None, dtype, nper, p, keep, p_path, path_keep)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["constant", "offset", "spike", "zero_gamma"])
def test_hard_rows(kind, dtype):
    """Rows that are hard for the row statistics, as in tests/test_gpu_bertnorm.py, whose docstring says why the
    upstream gradients are positive here (a spike column makes dgamma_c a sum over rows that cancels under random signs
    and multiplies the half unit of rstd on either route)."""
    for rows, hidden in ((9, 192), (5, 65), (6, 1024)):
        x, b, gamma, beta, g_s, g_y = make_inputs(rows, hidden, "plain", dtype, seed=31 + hidden, kind=kind)
        compare(f"{kind} {rows}x{hidden}", x, b, gamma.to(DEV), beta.to(DEV), g_s.abs().to(dtype).to(DEV),
                g_y.abs().to(dtype).to(DEV), dtype, nper=rows)


def test_float16_is_forward_only():
    dtype = torch.float16
    for rows, hidden, layout in ((2 * 197, 192, "plain"), (5, 65, "odd"), (17, 384, "slice")):
        x, b, gamma, beta, g_s, g_y = make_inputs(rows, hidden, layout, dtype, seed=3)
        for pdt in (torch.float32, dtype):
            path_keep = torch.tensor([0] + [1] * (rows - 1), dtype=torch.uint8, device=DEV)
            compare("f16", x, b, gamma.to(pdt).to(DEV), beta.to(pdt).to(DEV), None, None, dtype, 1, 0.0, None, 0.5,
                    path_keep, grads=False)
    gamma, beta = gamma.to(DEV), beta.to(DEV)
    s, y, stats = ops.prenorm_fwd(x, b, gamma, beta, need_stats=True)
    with pytest.raises(_cabi.TadmmError, match="forward only"):
        ops.prenorm_bwd(s, gamma, stats, y, None)
    with pytest.raises(_cabi.TadmmError, match="float16 with gradients"):
        HF.add_layer_norm(x.detach().requires_grad_(), b, gamma, beta, route="launch")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_two_backward_runs_are_bit_identical(dtype):
    B, N, hidden = 21, 197, 192                        # 4137 rows: more than two trips of the backward's grid
    assert B * N > 2 * 4 * BWD_GRID
    x, b, gamma, beta, g_s, g_y = make_inputs(B * N, hidden, "plain", dtype, seed=5)
    gamma, beta, g_s, g_y = gamma.to(DEV), beta.to(DEV), g_s.to(dtype).to(DEV), g_y.to(dtype).to(DEV)
    keep = HF.residual_keep_mask((B, N, hidden), 0.1, DEV)
    path_keep = HF.drop_path_keep_mask(B, 0.3, DEV)
    other = make_inputs(33, 1000, "plain", dtype, seed=6)
    runs = []
    for n in range(2):
        leaves = [x.view(B, N, hidden).detach().requires_grad_(), b.view(B, N, hidden).detach().requires_grad_(),
                  gamma.detach().requires_grad_(), beta.detach().requires_grad_()]
        s, y = HF.add_layer_norm(*leaves, dropout_p=0.1, drop_path_p=0.3, training=True, keep=keep, path_keep=path_keep,
                                 route="launch")
        runs.append((s, y) + torch.autograd.grad([s, y], leaves, [g_s.view(B, N, hidden), g_y.view(B, N, hidden)]))
        if n == 0:                                     # a call of another shape in between
            o = [t.to(DEV).requires_grad_() if t.device.type == "cpu" else t.detach().requires_grad_() for t in other[:4]]
            so, yo = HF.add_layer_norm(*o, route="launch")
            (so.sum() + yo.sum()).backward()
    for a, c in zip(*runs):
        assert torch.equal(a, c)
    assert runs[0][2].untyped_storage().data_ptr() != runs[0][3].untyped_storage().data_ptr()


def test_masks_follow_the_seed_and_wide_rows_take_the_composed_route():
    x, b = torch.randn(4, 37, 96, device=DEV), torch.randn(4, 37, 96, device=DEV)
    w, beta = torch.rand(96, device=DEV) + 0.5, torch.rand(96, device=DEV)
    outs = []
    for seed in (11, 11, 12):
        torch.manual_seed(seed)
        outs.append(HF.add_layer_norm(x, b, w, beta, dropout_p=0.2, drop_path_p=0.5, training=True, route="launch"))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], outs[2][0])
    ev = HF.add_layer_norm(x, b, w, beta, dropout_p=0.2, drop_path_p=0.5, training=False, route="launch")
    assert torch.equal(ev[0], x + b)
    wide, wb = torch.randn(3, HMAX + 8, device=DEV), torch.randn(3, HMAX + 8, device=DEV)
    w, beta = torch.ones(HMAX + 8, device=DEV), torch.zeros(HMAX + 8, device=DEV)
    for got, want in zip(HF.add_layer_norm(wide, wb, w, beta), HF.add_layer_norm_composed(wide, wb, w, beta)):
        assert torch.equal(got, want)
    with pytest.raises(_cabi.TadmmError):
        HF.add_layer_norm(wide, wb, w, beta, route="launch")
    t = torch.randn(4, 6, 80, device=DEV)[:, ::2, ::2]                # no unit element stride: copied
    w, beta = torch.rand(40, device=DEV), torch.rand(40, device=DEV)
    for got, want in zip(HF.add_layer_norm(t, t, w, beta, route="launch"), HF.add_layer_norm_composed(t, t, w, beta)):
        assert torch.allclose(got, want, atol=1e-5)
