"""The saving launches of the fused chains (csrc/chain.hip, SAVE): `tadmm_ttlinear_fwd_save` / `_bwd_save` on token rows,
`tadmm_svdconv_fwd_save` / `_bwd_save` on NCHW images, and the training route of `tadmm.functional` built on them.

Shapes: T = 70 token rows (ragged for the 32- and the 64-token tile), K = 40, ranks 20 / 72 / 200 (padded to 64 / 128 /
256, none a multiple of 16), output widths 24 / 72; images of batch 2 with planes of 49 (element stores) and 64 pixels
(16-byte stores).  Three to five workgroups reach every edge.

Bounds: the stored intermediate is ONE product, so it is judged elementwise by the one-product bounds already in the
tree -- `linear_bound` of tests/_fp16_ref.py with u = 2^-8 for bfloat16, `linear_bound_f32` of tests/_chain_ref.py for
float32 -- through `bound_of`.  The gradient tolerances are those tests/test_gpu_chain.py and tests/test_gpu_svd_layers.py
apply to the same gradients on the recomputing route: 1e-5 of the largest reference entry for dX and the bias (and for
the image weights), 2e-5 for the factors of the token-row chain; bfloat16 is held to the 2e-2 those files state for
the bfloat16 mode.  Between the routes dX is bitwise equal and a weight gradient differs by at most the sum of the two
routes' tolerances."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from _chain_ref import SENTINEL, bound_of, guarded, guards_intact, image_rows, same_bits, untouched

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, K = 70, 40
ERR_INVALID = -1
DTYPES = [torch.float32, torch.bfloat16]


def _mods():
    from tadmm import _cabi, ops
    return _cabi, ops


def _launch(entry, X, Y, win, wout, bias, Tn, kin, rpad, nout, ldx=0, ldy=0, hw=0, tile=0, dtype=None, save=None):
    """Raw C ABI call.  `save` = (true rank, h pointer or tensor or None, ldh) selects the six-argument form."""
    _cabi, ops = _mods()
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())   # noqa: E731
    d = _cabi.ChainDesc()
    d.X, d.Y, d.Win, d.Wout, d.bias = ptr(X), ptr(Y), ptr(win), ptr(wout), ptr(bias)
    d.T, d.Kin, d.R, d.Nout = Tn, kin, rpad, nout
    d.ldx, d.ldy = ldx, ldy
    d.win_plane, d.wout_plane = win[0].numel(), wout[0].numel()
    d.x_hw, d.y_hw, d.tile_tokens = hw, hw, tile
    if dtype is None:
        dtype = {torch.float32: _cabi.CHAIN_F32, torch.bfloat16: _cabi.CHAIN_BF16, torch.float16: _cabi.CHAIN_F16}[X.dtype]
    d.dtype = dtype
    h = ops.Handle.get(torch.cuda.current_device())
    stream = torch.cuda.current_stream().cuda_stream
    if save is None:
        return getattr(h.lib, entry)(h.ptr, C.byref(d), stream), h
    r, hp, ldh = save
    return getattr(h.lib, entry)(h.ptr, C.byref(d), r, ptr(hp), ldh, stream), h


def _operands(r, n, dtype, seed):
    """x (T, K), dY (T, n), Win (r, K), Wout (n, r), bias; weights as the kernel multiplies them (rounded for bfloat16)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, K, generator=g).to(DEV).to(dtype)
    gy = torch.randn(T, n, generator=g).to(DEV).to(dtype)
    win = (torch.randn(r, K, generator=g) / K ** 0.5).to(DEV)
    wout = (torch.randn(n, r, generator=g) / r ** 0.5).to(DEV)
    bias = torch.randn(n, generator=g).to(DEV)
    if dtype == torch.bfloat16:
        win, wout = win.bfloat16().float(), wout.bfloat16().float()
    return x, gy, win, wout, bias


def _planes(w_first, w_second, dtype):
    _, ops = _mods()
    P = 3 if dtype == torch.float32 else 1
    return ops.weight_planes(w_first, P, pad_rows=64), ops.weight_planes(w_second, P, pad_cols=64)


def _check_h(name, h, x_rows, w, dtype):
    ref, bound = bound_of(x_rows, [w], None, dtype)
    err = (h.double() - ref).abs()
    worst = (err / bound).max().item()
    print(f"{name}: worst err / bound {worst:.3f}, max err / max|ref| {err.max().item() / ref.abs().max().item():.3e}")
    assert torch.isfinite(h.float()).all() and worst <= 1.0, (name, worst)


# ------------------------------------------------------------------------------------------------ token rows
@pytest.mark.parametrize("tile", [32, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [24, 72])
@pytest.mark.parametrize("r", [20, 72, 200])
def test_rows_save_entries(r, n, dtype, tile):
    x, gy, win, wout, bias = _operands(r, n, dtype, 100 * r + n)
    rpad = -(-r // 64) * 64
    # (entry pair, X, first factor (r, kin), second factor (nout, r), bias)
    for plain, save, X, w1, w2, b in (("tadmm_ttlinear_fwd", "tadmm_ttlinear_fwd_save", x, win, wout, bias),
                                      ("tadmm_ttlinear_bwd", "tadmm_ttlinear_bwd_save", gy, wout.t(), win.t(), None)):
        p1, p2 = _planes(w1, w2, dtype)
        kin, nout = X.shape[1], w2.shape[0]
        y0 = torch.empty(T, nout, dtype=dtype, device=DEV)
        rc, _ = _launch(plain, X, y0, p1, p2, b, T, kin, rpad, nout, ldx=kin, ldy=nout, tile=tile)
        assert rc == 0
        # ldh = r + 3: element stores (no 16-byte phase survives an odd stride); a stride of whole units: vector stores
        for ldh in (r + 3, -(-r // 8) * 8 + 8):
            y1 = torch.empty(T, nout, dtype=dtype, device=DEV)
            h = guarded((T, r), dtype, ld=ldh)
            rc, _ = _launch(save, X, y1, p1, p2, b, T, kin, rpad, nout, ldx=kin, ldy=nout, tile=tile, save=(r, h, ldh))
            assert rc == 0
            assert same_bits(y0, y1), (save, ldh)                # the save is extra stores, not another summation
            assert guards_intact(h), (save, ldh)                  # nothing outside (T, r): not [r, padded rank), not the gaps
            assert not bool((h == SENTINEL).any())
            _check_h(f"{save} r={r} n={n} tile={tile} ldh={ldh}", h, X, w1, dtype)


# ------------------------------------------------------------------------------------------------ images
@pytest.mark.parametrize("tile", [32, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("hw", [(7, 7), (8, 8)], ids=["49px", "64px"])
@pytest.mark.parametrize("r,n", [(20, 72), (72, 24), (200, 72)])
def test_image_save_entries(r, n, hw, dtype, tile):
    B, (H, W) = 2, hw
    px = H * W
    g = torch.Generator().manual_seed(7 * r + n + px)
    x = torch.randn(B, K, H, W, generator=g).to(DEV).to(dtype)
    gy = torch.randn(B, n, H, W, generator=g).to(DEV).to(dtype)
    win = (torch.randn(r, K, generator=g) / K ** 0.5).to(DEV)
    wout = (torch.randn(n, r, generator=g) / r ** 0.5).to(DEV)
    bias = torch.randn(n, generator=g).to(DEV)
    if dtype == torch.bfloat16:
        win, wout = win.bfloat16().float(), wout.bfloat16().float()
    rpad = -(-r // 64) * 64
    for plain, save, X, w1, w2, b in (("tadmm_svdconv_fwd", "tadmm_svdconv_fwd_save", x, win, wout, bias),
                                      ("tadmm_svdconv_bwd", "tadmm_svdconv_bwd_save", gy, wout.t(), win.t(), None)):
        p1, p2 = _planes(w1, w2, dtype)
        kin, nout = X.shape[1], w2.shape[0]
        y0 = torch.empty(B, nout, H, W, dtype=dtype, device=DEV)
        rc, _ = _launch(plain, X, y0, p1, p2, b, B * px, kin, rpad, nout, hw=px, tile=tile)
        assert rc == 0
        y1 = torch.empty_like(y0)
        buf = guarded((B, r + 1, H, W), dtype)                    # one guard channel behind the r stored ones
        rc, _ = _launch(save, X, y1, p1, p2, b, B * px, kin, rpad, nout, hw=px, tile=tile, save=(r, buf, r + 1))
        assert rc == 0
        assert same_bits(y0, y1), save
        assert guards_intact(buf) and untouched(buf[:, r]), save
        h = buf[:, :r]
        assert not bool((h == SENTINEL).any())
        _check_h(f"{save} r={r} n={n} {px}px tile={tile}", image_rows(h), image_rows(X), w1, dtype)


# ------------------------------------------------------------------------------------------------ refusals
def test_save_entries_refuse_without_writing():
    _cabi, ops = _mods()
    r, n, rpad = 20, 24, 64

    def expect_invalid(entry, X, p1, p2, nout, hshape, hw=0, Tn=T, ld=None, save_of=None, dtype=None):
        y = torch.full((Tn, nout) if hw == 0 else (X.shape[0], nout, *X.shape[2:]), SENTINEL, dtype=X.dtype, device=DEV)
        h = guarded(hshape, X.dtype, ld=ld)
        kin = X.shape[1]
        rc, hd = _launch(entry, X, y, p1, p2, None, Tn, kin, rpad, nout, ldx=0 if hw else kin, ldy=0 if hw else nout, hw=hw,
                         dtype=dtype, save=save_of(h))
        torch.cuda.synchronize()
        assert rc == ERR_INVALID, (entry, rc)
        assert hd.lib.tadmm_last_error(hd.ptr).decode() != ""
        assert untouched(y) and untouched(h) and guards_intact(h), entry
        return hd.lib.tadmm_last_error(hd.ptr).decode()

    for dtype in DTYPES:
        x, gy, win, wout, _ = _operands(r, n, dtype, 3)
        esz = x.element_size()
        for entry, X, w1, w2 in (("tadmm_ttlinear_fwd_save", x, win, wout), ("tadmm_ttlinear_bwd_save", gy, wout.t(), win.t())):
            p1, p2 = _planes(w1, w2, dtype)
            nout = w2.shape[0]
            assert "null h_out" in expect_invalid(entry, X, p1, p2, nout, (T, r), save_of=lambda h: (r, None, r))
            assert "ldh" in expect_invalid(entry, X, p1, p2, nout, (T, r), save_of=lambda h: (r, h, r - 1))
            assert "aligned" in expect_invalid(entry, X, p1, p2, nout, (T, r), ld=r + 3,
                                               save_of=lambda h: (r, h.data_ptr() + esz // 2, r + 3))
            assert "rank" in expect_invalid(entry, X, p1, p2, nout, (T, r), save_of=lambda h: (rpad + 1, h, rpad + 1))
        # images: a partial last plane (T % hw != 0) is refused as the plain entry refuses it
        xi = torch.randn(2, K, 7, 7, device=DEV).to(dtype)
        p1, p2 = _planes(win, wout, dtype)
        for entry in ("tadmm_svdconv_fwd_save", "tadmm_svdconv_bwd_save"):
            assert "whole number of planes" in expect_invalid(entry, xi, p1, p2, n, (2, r, 7, 7), hw=49, Tn=97,
                                                              save_of=lambda h: (r, h, r))
            assert "null h_out" in expect_invalid(entry, xi, p1, p2, n, (2, r, 7, 7), hw=49, Tn=98,
                                                  save_of=lambda h: (r, None, r))
            assert "ldh" in expect_invalid(entry, xi, p1, p2, n, (2, r, 7, 7), hw=49, Tn=98, save_of=lambda h: (r, h, r - 1))
    # binary16: inference only -- there is no binary16 weight gradient to feed
    x16 = torch.randn(T, K, device=DEV).half()
    g = torch.Generator().manual_seed(5)
    win, wout = torch.randn(r, K, generator=g).to(DEV), torch.randn(n, r, generator=g).to(DEV)
    p1 = ops.weight_planes(win, 1, pad_rows=64, dtype=torch.float16)
    p2 = ops.weight_planes(wout, 1, pad_cols=64, dtype=torch.float16)
    for entry in ("tadmm_ttlinear_fwd_save", "tadmm_ttlinear_bwd_save"):
        assert "binary16" in expect_invalid(entry, x16, p1, p2, n, (T, r), save_of=lambda h: (r, h, r))
    xi16 = torch.randn(2, K, 8, 8, device=DEV).half()
    for entry in ("tadmm_svdconv_fwd_save", "tadmm_svdconv_bwd_save"):
        assert "binary16" in expect_invalid(entry, xi16, p1, p2, n, (2, r, 8, 8), hw=64, Tn=128, save_of=lambda h: (r, h, r))
    with pytest.raises(_cabi.TadmmError):                         # and through the wrapper
        ops.chain_fused_save(x16, p1, p2, None, n, r)


# ------------------------------------------------------------------------------------------------ autograd
def _rel(a, ref):
    return (a.double() - ref.double()).abs().max().item() / max(ref.double().abs().max().item(), 1e-30)


def _run_route(fn, leaves, gout, save):
    ls = [None if t is None else t.detach().clone().requires_grad_() for t in leaves]
    y = fn(*ls, save=save)
    (y * gout).sum().backward()
    return y.detach(), [None if t is None else t.grad for t in ls]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("image", [False, True], ids=["rows", "images"])
def test_autograd_saved_route_matches_fp64_and_the_other_route(image, bias, dtype):
    from tadmm import functional as HF
    r, n = 20, 72
    g = torch.Generator().manual_seed(11 + image + 2 * bias)
    x = torch.randn(*((3, K, 7, 7) if image else (T, K)), generator=g).to(DEV).to(dtype)
    wi = (torch.randn(r, K, generator=g) / K ** 0.5).to(DEV)
    wo = (torch.randn(n, r, generator=g) / r ** 0.5).to(DEV)
    b = torch.randn(n, generator=g).to(DEV) if bias else None
    gout = torch.randn(*((3, n, 7, 7) if image else (T, n)), generator=g).to(DEV).to(dtype)
    fn = HF.conv1x1_chain if image else HF.linear_chain
    y1, g1 = _run_route(fn, (x, wi, wo, b), gout, True)
    y0, g0 = _run_route(fn, (x, wi, wo, b), gout, False)
    l64 = [None if t is None else t.detach().double().requires_grad_() for t in (x, wi, wo, b)]
    if image:
        y64 = F.conv2d(F.conv2d(l64[0], l64[1][:, :, None, None]), l64[2][:, :, None, None], l64[3])
    else:
        y64 = F.linear(F.linear(l64[0], l64[1]), l64[2], l64[3])
    (y64 * gout.double()).sum().backward()
    if dtype == torch.float32:
        tol = {"dX": 1e-5, "dWin": 1e-5 if image else 2e-5, "dWout": 1e-5 if image else 2e-5, "dbias": 1e-5}
    else:
        tol = dict.fromkeys(("dX", "dWin", "dWout", "dbias"), 2e-2)
    assert same_bits(y0, y1) and same_bits(g0[0], g1[0])          # y and dX: the same launches' arithmetic, bit for bit
    for what, a1, a0, ref in zip(("dX", "dWin", "dWout", "dbias"), g1, g0, l64):
        if a1 is None:
            continue
        e1, e0, between = _rel(a1, ref.grad), _rel(a0, ref.grad), _rel(a1, a0)
        print(f"{what} {dtype} image={image}: saved {e1:.2e}, recomputed {e0:.2e}, between {between:.2e}, tol {tol[what]:.0e}")
        assert e1 < tol[what], (what, e1)
        assert between <= 2 * tol[what] * ref.grad.abs().max().item() / a0.double().abs().max().item(), (what, between)


def _count(monkeypatch, ops):
    calls = []
    for name in ("chain_fused", "chain_fused_save", "svd_conv", "svd_conv_save", "chain_single", "wgrad"):
        real = getattr(ops, name)

        def wrapped(*a, _real=real, _name=name, **k):
            calls.append((_name, k.get("entry")))
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)
    return calls


@pytest.mark.parametrize("image", [False, True], ids=["rows", "images"])
def test_launches_of_a_step(monkeypatch, image):
    from tadmm import functional as HF, ops
    calls = _count(monkeypatch, ops)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(*((2, K, 8, 8) if image else (T, K)), generator=g).to(DEV)
    wi, wo = torch.randn(20, K, generator=g).to(DEV), torch.randn(24, 20, generator=g).to(DEV)
    b = torch.randn(24, generator=g).to(DEV)
    fn = HF.conv1x1_chain if image else HF.linear_chain
    plain, save = ("svd_conv", "svd_conv_save") if image else ("chain_fused", "chain_fused_save")
    bwd = "tadmm_svdconv_bwd" if image else "tadmm_ttlinear_bwd"
    # every factor wants a gradient: _fwd_save, _bwd_save, two weight gradients, nothing recomputed
    ls = [t.clone().requires_grad_() for t in (x, wi, wo, b)]
    fn(*ls, save=True).sum().backward()
    assert calls == [(save, None), (save, bwd + "_save"), ("wgrad", None), ("wgrad", None)], calls
    # only x wants a gradient: nothing is saved, the plain entries run
    del calls[:]
    xg = x.clone().requires_grad_()
    fn(xg, wi, wo, b, save=True).sum().backward()
    assert calls == [(plain, None), (plain, bwd)], calls
    # the other route, forced: the parent's launches
    del calls[:]
    ls = [t.clone().requires_grad_() for t in (x, wi, wo, b)]
    fn(*ls, save=False).sum().backward()
    assert [c[0] for c in calls] == [plain, plain, "chain_single", "wgrad", "chain_single", "wgrad"], calls
    # only the output factor wants a gradient: H is saved, no data-gradient launch at all
    del calls[:]
    wog = wo.clone().requires_grad_()
    fn(x, wi, wog, b, save=True).sum().backward()
    assert calls == [(save, None), ("wgrad", None)], calls


# ------------------------------------------------------------------------------------------------ layers
class _HP:
    pass


def _sgd_step_and_check(params, refs, lr=0.1):
    before = [p.detach().clone() for p in params]
    torch.optim.SGD(params, lr=lr).step()
    for p, p0, what in zip(params, before, refs):
        assert p.grad is not None and bool((p.grad != 0).any()), what
        torch.testing.assert_close(p.detach(), p0 - lr * p.grad, rtol=1e-6, atol=1e-8, msg=what)


def test_ttlinearm_step_on_the_saved_route(monkeypatch):
    from tadmm import ops, tt_layers
    torch.manual_seed(1)
    hp = _HP()
    hp.tt_shapes = {"w": [8, 6, 4, 12]}
    hp.ranks = {"w": [1, 5, 20, 6, 1]}
    lin = tt_layers.TTLinearM(48, 48, bias=True, hp_dict=hp, name="w").cuda()
    monkeypatch.setattr(ops, "chain_train_pays", lambda *a, **k: True)
    calls = _count(monkeypatch, ops)
    x = torch.randn(T, 48, device=DEV, requires_grad=True)
    y = lin(x)
    gy = torch.randn_like(y)
    y.backward(gy)
    names = [c[0] for c in calls]
    assert names.count("chain_fused_save") == 2 and "chain_single" not in names and "chain_fused" not in names, calls
    cores = [c.detach().double().requires_grad_(True) for c in lin.tt_cores]
    w = cores[0].reshape(-1, cores[0].shape[-1])
    for c in cores[1:]:
        w = w.reshape(-1, c.shape[0]) @ c.reshape(c.shape[0], -1)
    xd = x.detach().double().requires_grad_(True)
    bd = lin.bias.detach().double().requires_grad_(True)
    yd = xd @ w.reshape(48, 48).t() + bd
    yd.backward(gy.double())
    assert _rel(y.detach(), yd.detach()) < 1e-5
    assert _rel(x.grad, xd.grad) < 1e-5 and _rel(lin.bias.grad, bd.grad) < 1e-5
    for c, cd in zip(lin.tt_cores, cores):
        assert _rel(c.grad, cd.grad) < 2e-5
    _sgd_step_and_check(list(lin.parameters()), [n for n, _ in lin.named_parameters()])


def test_tklinearm_step_on_the_saved_route(monkeypatch):
    from tadmm import ops, tk_layers
    torch.manual_seed(5)
    hk = _HP()
    hk.ranks = {"k.weight": [40, 24]}
    lin = tk_layers.TKLinearM(96, 128, bias=True, hp_dict=hk, name="k.weight").cuda()
    with torch.no_grad():
        lin.bias.normal_()
    monkeypatch.setattr(ops, "chain_train_pays", lambda *a, **k: True)
    calls = _count(monkeypatch, ops)
    x = torch.randn(T, 96, device=DEV, requires_grad=True)
    y = lin(x)
    gy = torch.randn_like(y)
    y.backward(gy)
    names = [c[0] for c in calls]
    assert names.count("chain_fused_save") == 2 and "chain_single" not in names and "chain_fused" not in names, calls
    ps = (lin.first_factor, lin.core_tensor, lin.last_factor, lin.bias)
    params = [p.detach().double().requires_grad_(True) for p in ps]
    xd = x.detach().double().requires_grad_(True)
    yd = xd @ (params[2] @ params[1] @ params[0]).t() + params[3]
    yd.backward(gy.double())
    assert _rel(x.grad, xd.grad) < 1e-5
    for p, pd in zip(ps, params):
        assert _rel(p.grad, pd.grad) < 2e-5
    _sgd_step_and_check(list(lin.parameters()), [n for n, _ in lin.named_parameters()])
