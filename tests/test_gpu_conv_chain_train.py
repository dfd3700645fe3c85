"""Training on the one-launch factorised convolution (csrc/convchain.hip): the forward that also stores H1 / H2
(`tadmm_ttconv_fused_save`), the one-launch data gradient with dH1 / dH2 (`tadmm_ttconv_fused_bwd`), the autograd
Function `functional.conv_chain` and the three factorised layers forced onto it, against the float64 composition
1x1 -> k x k -> 1x1 + bias and its autograd.

Bars (max error over max |reference|): 1e-5 for fp32 Y, dX and the saved intermediates; 3e-2 for bf16 Y, dX and
intermediates against the reference of the bf16-rounded operands (the bar of tests/test_gpu_chain.py); 1e-5 for the
weight gradients in both dtypes against the float64 products of the tensors the weight-gradient kernels read (the saved
intermediates: the bar of tests/test_gpu_wgrad.py and tests/test_gpu_core_conv.py); 2e-5 / 2e-2 for the forced layers in
fp32 / bf16 autocast (the bars of tests/test_gpu_core_conv.py)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from _unaligned import SENTINEL
from test_gpu_core_conv import _layers, _reference, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


@functools.lru_cache(maxsize=None)
def _operands(C_, O, r1, r2, hw, k, s, p, dl, dtype, seed=0, B=2):
    """Operands of `dtype` and the float64 reference of the rounded operands (computed once per case, never modified)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    k = _pair(k)
    x = torch.randn(B, C_, *hw, generator=g).to(DEV).to(dtype)
    w1 = (torch.randn(r1, C_, generator=g) * C_ ** -0.5).to(DEV)
    core = (torch.randn(r2, r1, *k, generator=g) * (r1 * k[0] * k[1]) ** -0.5).to(DEV)
    w3 = (torch.randn(O, r2, generator=g) * r2 ** -0.5).to(DEV)
    bias = torch.randn(O, generator=g).to(DEV)
    if dtype == torch.bfloat16:
        w1, core, w3 = (t.bfloat16().float() for t in (w1, core, w3))     # the one plane the kernel multiplies with
    x64 = x.double().requires_grad_()
    h1 = F.conv2d(x64, w1.double()[:, :, None, None])
    h2 = F.conv2d(h1, core.double(), None, s, p, dl)
    y64 = F.conv2d(h2, w3.double()[:, :, None, None], bias.double())
    dy = torch.randn(y64.shape, generator=g).to(DEV).to(dtype)
    dx64, dh1, dh2 = torch.autograd.grad(y64, (x64, h1, h2), dy.double())
    # input pixels some tap of some output pixel reads
    reach = torch.autograd.grad(F.conv2d(x64[:1, :1], torch.ones(1, 1, *k, device=DEV, dtype=torch.float64), None, s, p, dl).sum(),
                                x64, allow_unused=False)[0][0, 0] != 0
    ref = dict(y=y64.detach(), dx=dx64, h1=h1.detach() * reach, h2=h2.detach(), dh1=dh1, dh2=dh2, reach=reach)
    return x, w1, core, w3, bias, dy, ref


def _planes(w1, core, w3, dtype):
    from tadmm import ops
    n = 3 if dtype == torch.float32 else 1
    fwd = (ops.weight_planes(w1, n, pad_rows=32), ops.conv_core_planes(core, n), ops.weight_planes(w3, n))
    bwd = (ops.weight_planes(w3.t(), n, pad_rows=32), ops.conv_core_planes(core.permute(1, 0, 2, 3), n), ops.weight_planes(w1.t(), n))
    return fwd, bwd


def _guarded(shape, dtype, off=0):
    """An output tensor of `shape` at element offset `off` past a 16-byte boundary inside a sentinel-filled buffer."""
    n = 1
    for v in shape:
        n *= v
    buf = torch.full((n + 24,), SENTINEL, dtype=dtype, device=DEV)
    v = buf[8 + off:8 + off + n].view(shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == (off * buf.element_size()) % 16
    return v


def _guards_intact(v):
    base, s, n = v._base, v.storage_offset(), v.numel()
    want = torch.tensor(SENTINEL, dtype=v.dtype, device=v.device)
    return bool((base[:s] == want).all()) and bool((base[s + n:] == want).all())


def _run(case, dtype, off=0):
    """Forward + save and backward + save into guarded outputs; returns the nine results."""
    from tadmm import ops
    C_, O, r1, r2, hw, k, s, p, dl = case
    k, s, p, dl = _pair(k), _pair(s), _pair(p), _pair(dl)
    x, w1, core, w3, bias, dy, ref = _operands(*case, dtype)
    if off:
        xo, dyo = _guarded(x.shape, dtype, off), _guarded(dy.shape, dtype, off)
        xo.copy_(x), dyo.copy_(dy)
        x, dy = xo, dyo
    fwd, bwd = _planes(w1, core, w3, dtype)
    B = x.shape[0]
    ho, wo = ref["y"].shape[2:]
    outs_f = (_guarded((B, O, ho, wo), dtype, off), _guarded((B, r1, *hw), dtype, off), _guarded((B, r2, ho, wo), dtype, off))
    outs_b = (_guarded(x.shape, dtype, off), _guarded((B, r1, *hw), dtype, off), _guarded((B, r2, ho, wo), dtype, off))
    y, h1, h2 = ops.conv_chain_save(x, *fwd, bias, O, r1, r2, k, s, p, dl, out=outs_f)
    dx, dh1, dh2 = ops.conv_chain_bwd(dy, *bwd, x.shape, r1, r2, k, s, p, dl, save=True, out=outs_b)
    dw3 = ops.wgrad(dy, h2)
    dw1 = ops.wgrad(dh1, x)
    dwc = ops.core_conv_wgrad(dh2, h1, k, s, p, dl)
    for t in outs_f + outs_b + ((x, dy) if off else ()):
        assert _guards_intact(t)
    return dict(y=y, h1=h1, h2=h2, dx=dx, dh1=dh1, dh2=dh2, dw3=dw3, dw1=dw1, dwc=dwc), (x, dy)


def _check(case, dtype, off=0):
    C_, O, r1, r2, hw, k, s, p, dl = case
    x, w1, core, w3, bias, dy, ref = _operands(*case, dtype)
    got, (xu, dyu) = _run(case, dtype, off)
    bar = 1e-5 if dtype == torch.float32 else 3e-2
    errs = {n: _rel(got[n], ref[n]) for n in ("y", "dx", "h1", "h2", "dh1", "dh2")}
    # weight gradients: float64 products of what the weight-gradient kernels read
    h1, h2, dh1, dh2 = (got[n].double() for n in ("h1", "h2", "dh1", "dh2"))
    c64 = core.double().requires_grad_()
    dwc64 = torch.autograd.grad(F.conv2d(h1, c64, None, s, p, dl), c64, dh2)[0]
    errs["dw3"] = _rel(got["dw3"], torch.einsum("bohw,brhw->or", dy.double(), h2))
    errs["dw1"] = _rel(got["dw1"], torch.einsum("brhw,bchw->rc", dh1, x.double()))
    errs["dwc"] = _rel(got["dwc"], dwc64)
    print(f"conv-chain-train {case} {dtype} off={off}: " + " ".join(f"{n} {e:.3e}" for n, e in errs.items()))
    for n in ("y", "dx", "h1", "h2", "dh1", "dh2"):
        assert got[n].dtype == dtype and got[n].shape == ref[n].shape
        assert errs[n] < bar, (n, errs[n])
    for n in ("dw3", "dw1", "dwc"):
        assert got[n].dtype == torch.float32 and errs[n] < 1e-5, (n, errs[n])
    # pixels no tap reaches: exact zeros in dX and in the stored H1
    miss = ~ref["reach"]
    if miss.any():
        assert got["dx"][:, :, miss].abs().max().item() == 0.0
        assert got["h1"][:, :, miss].abs().max().item() == 0.0
    return got


RAGGED = (24, 40, 20, 28)
CASES = {
    "1-one-tile": (*RAGGED, (7, 7), 3, 1, 1, 1),
    "2-stride2-4+4+4+2": (*RAGGED, (14, 14), 3, 2, 1, 1),
    "3-28x28-shared-halos": (*RAGGED, (28, 28), 3, 1, 1, 1),
    "4-56x56-row-per-tile": (8, 8, 12, 20, (56, 56), 3, 1, 1, 1),
    "5-1x1-stride2-unreached": (*RAGGED, (8, 8), 1, 2, 0, 1),
    "6-3x3-stride2-pad0-unreached-edge": (*RAGGED, (8, 8), 3, 2, 0, 1),
    "7-5x5-dilation2": (*RAGGED, (9, 9), 5, 1, 2, 2),
    "8-1x3-nonsquare": (*RAGGED, (6, 10), (1, 3), 1, (0, 1), 1),
    "w64": (8, 8, 12, 20, (2, 64), 3, 1, 1, 1),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_kernels_match_fp64(name, dtype):
    from tadmm import ops
    case = CASES[name]
    C_, O, r1, r2, hw, k, s, p, dl = case
    x = _operands(*case, dtype)[0]
    geom = (_pair(k), _pair(s), _pair(p), _pair(dl))
    assert ops.conv_chain_fits(x, r1, r2, *geom) and ops.conv_chain_bwd_fits(x, r1, r2, *geom)
    if name.startswith("2-"):
        assert ops._conv_chain_bwd_plan(tuple(x.shape), dtype, r1, r2, *geom)[1:] == (4, 1, 4)    # dX tiles of 4+4+4+2 rows
    if name.startswith("3-"):
        assert ops._conv_chain_plan(x, r1, r2, *geom)[3] == 14
    if name.startswith("4-"):
        assert ops._conv_chain_bwd_plan(tuple(x.shape), dtype, r1, r2, *geom)[1] == 1
    _check(case, dtype)


@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("name", ["1-one-tile", "3-28x28-shared-halos", "6-3x3-stride2-pad0-unreached-edge"])
def test_unaligned_fp32_operands_and_outputs(name, off):
    """Every tensor at element offset 1 / 3 of a sentinel-filled buffer: same bars, same bits as the aligned call."""
    got = _check(CASES[name], torch.float32, off)
    ref, _ = _run(CASES[name], torch.float32, 0)
    for n in got:
        assert torch.equal(got[n], ref[n]), n


def test_rank_bound():
    """r1 = r2 = 256 is the largest rank (bf16: the fp32 planes of 256 channels leave the LDS under the forward's tile
    rule, which this feature does not change); 264 is refused and `fits` says so."""
    from tadmm import ops
    from tadmm._cabi import TadmmError
    case = (24, 40, 256, 256, (7, 7), 3, 1, 1, 1)
    _check(case, torch.bfloat16)
    geom = ((3, 3), (1, 1), (1, 1), (1, 1))
    x32 = torch.zeros(2, 24, 7, 7, device=DEV)
    assert not ops.conv_chain_fits(x32, 256, 256, *geom) and not ops.conv_chain_bwd_fits(x32, 256, 256, *geom)
    for dtype in (torch.float32, torch.bfloat16):
        x = x32.to(dtype)
        assert not ops.conv_chain_fits(x, 264, 264, *geom) and not ops.conv_chain_bwd_fits(x, 264, 264, *geom)
        big = (24, 40, 264, 264, (7, 7), 3, 1, 1, 1)
        xb, w1, core, w3, bias, dy, _ = _operands(*big, dtype)
        fwd, bwd = _planes(w1, core, w3, dtype)
        with pytest.raises(TadmmError) as e:
            ops.conv_chain_save(xb, *fwd, bias, 40, 264, 264, *geom)
        assert e.value.status == -5
        with pytest.raises(TadmmError) as e:
            ops.conv_chain_bwd(dy, *bwd, xb.shape, 264, 264, *geom)
        assert e.value.status == -5


def test_lds_need_forces_the_32_pixel_tile():
    from tadmm import ops
    case = (24, 40, 220, 220, (8, 8), 3, 1, 1, 1)
    x = _operands(*case, torch.float32)[0]
    geom = ((3, 3), (1, 1), (1, 1), (1, 1))
    assert ops._conv_chain_plan(x, 220, 220, *geom)[0] == 32
    assert ops._conv_chain_bwd_plan(tuple(x.shape), torch.float32, 220, 220, *geom)[0] == 32
    _check(case, torch.float32)


def test_determinism():
    for dtype in (torch.float32, torch.bfloat16):
        a, _ = _run(CASES["3-28x28-shared-halos"], dtype)
        b, _ = _run(CASES["3-28x28-shared-halos"], dtype)
        for n in a:
            assert torch.equal(a[n], b[n]), (n, dtype)


def test_widths():
    """Forward output width 65 is refused; with W = 65 and Wo = 33 the forward fits, the one-launch data gradient does not,
    and `functional.conv_chain` still returns correct gradients through the three-launch fallback."""
    from tadmm import functional as HF
    from tadmm import ops
    from tadmm._cabi import TadmmError
    geom1 = ((3, 3), (1, 1), (1, 1), (1, 1))
    wide = torch.zeros(2, 8, 2, 65, device=DEV)
    assert not ops.conv_chain_fits(wide, 12, 20, *geom1)
    with pytest.raises(TadmmError):
        HF.conv_chain(wide, torch.zeros(12, 8, device=DEV), torch.zeros(20, 12, 3, 3, device=DEV), torch.zeros(8, 20, device=DEV),
                      None, 1, 1, 1)
    case = (8, 8, 12, 20, (2, 65), 3, 2, 1, 1)
    geom2 = ((3, 3), (2, 2), (1, 1), (1, 1))
    x, w1, core, w3, bias, dy, ref = _operands(*case, torch.float32)
    assert ops.conv_chain_fits(x, 12, 20, *geom2) and not ops.conv_chain_bwd_fits(x, 12, 20, *geom2)
    fwd, bwd = _planes(w1, core, w3, torch.float32)
    with pytest.raises(TadmmError) as e:
        ops.conv_chain_bwd(dy, *bwd, x.shape, 12, 20, *geom2)
    assert e.value.status == -5
    leaves = [t.clone().requires_grad_() for t in (x, w1, core, w3, bias)]
    y = HF.conv_chain(*leaves, 2, 1, 1)
    grads = torch.autograd.grad(y, leaves, dy)
    l64 = [t.detach().double().requires_grad_() for t in (x, w1, core, w3, bias)]
    y64 = F.conv2d(F.conv2d(F.conv2d(l64[0], l64[1][:, :, None, None]), l64[2], None, 2, 1, 1), l64[3][:, :, None, None], l64[4])
    g64 = torch.autograd.grad(y64, l64, dy.double())
    assert _rel(y, y64.detach()) < 1e-5
    for n, a, b in zip(("dx", "dw1", "dwc", "dw3", "db"), grads, g64):
        err = _rel(a, b)
        print(f"conv-chain fallback {n} err={err:.3e}")
        assert err < 2e-5, (n, err)


# ------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_frozen_factors_save_nothing_and_take_one_launch(dtype, monkeypatch):
    from tadmm import functional as HF
    from tadmm import ops
    case = CASES["2-stride2-4+4+4+2"]
    x, w1, core, w3, bias, dy, ref = _operands(*case, dtype)
    calls = []
    real = ops.conv_chain_bwd
    monkeypatch.setattr(ops, "conv_chain_bwd", lambda *a, **k: (calls.append(k.get("save")), real(*a, **k))[1])

    def no_save(*a, **k):
        raise AssertionError("the saving forward ran for frozen factors")
    monkeypatch.setattr(ops, "conv_chain_save", no_save)
    for fn in ("chain_single", "wgrad", "core_conv_wgrad", "core_conv_dgrad"):
        monkeypatch.setattr(ops, fn, no_save)
    xg = x.clone().requires_grad_()
    y = HF.conv_chain(xg, w1, core, w3, bias, 2, 1, 1)
    saved = y.grad_fn.saved_tensors
    assert len(saved) == 3 and {tuple(t.shape) for t in saved} == {tuple(w1.shape), tuple(core.shape), tuple(w3.shape)}
    y.backward(dy)
    assert calls == [False]                                       # one launch, nothing stored
    bar = 1e-5 if dtype == torch.float32 else 3e-2
    assert _rel(y, ref["y"]) < bar and _rel(xg.grad, ref["dx"]) < bar


def test_function_gradients_and_only_what_is_asked_for(monkeypatch):
    from tadmm import functional as HF
    from tadmm import ops
    case = CASES["6-3x3-stride2-pad0-unreached-edge"]
    x, w1, core, w3, bias, dy, ref = _operands(*case, torch.float32)
    l64 = [t.detach().double().requires_grad_() for t in (x, w1, core, w3, bias)]
    y64 = F.conv2d(F.conv2d(F.conv2d(l64[0], l64[1][:, :, None, None]), l64[2], None, 2, 0, 1), l64[3][:, :, None, None], l64[4])
    g64 = torch.autograd.grad(y64, l64, dy.double())
    for native in (False, True):
        monkeypatch.setattr(HF, "CONV_CHAIN_DWC_NATIVE", native)
        leaves = [t.clone().requires_grad_() for t in (x, w1, core, w3, bias)]
        grads = torch.autograd.grad(HF.conv_chain(*leaves, 2, 0, 1), leaves, dy)
        for n, a, b in zip(("dx", "dw1", "dwc", "dw3", "db"), grads, g64):
            assert a.dtype == torch.float32 and _rel(a, b) < 2e-5, (n, native, _rel(a, b))
    # only W3 wants a gradient: no data-gradient launch at all
    calls = []
    real = ops.conv_chain_bwd
    monkeypatch.setattr(ops, "conv_chain_bwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    w3g = w3.clone().requires_grad_()
    (g3,) = torch.autograd.grad(HF.conv_chain(x, w1, core, w3g, bias, 2, 0, 1), (w3g,), dy)
    assert calls == [] and _rel(g3, g64[3]) < 2e-5


# ------------------------------------------------------------------------------------------------ layers
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "autocast"])
@pytest.mark.parametrize("kind", ["ttm", "tkc", "tkm"])
def test_layers_forced_onto_the_one_launch_path(kind, bf16, with_bias, monkeypatch):
    from tadmm import functional as HF
    from tadmm import ops
    monkeypatch.setattr(ops, "conv_chain_train_pays", lambda *a, **k: True)
    calls = {"save": 0, "bwd": 0}
    real_s, real_b = ops.conv_chain_save, ops.conv_chain_bwd
    monkeypatch.setattr(ops, "conv_chain_save", lambda *a, **k: (calls.__setitem__("save", calls["save"] + 1), real_s(*a, **k))[1])
    monkeypatch.setattr(ops, "conv_chain_bwd", lambda *a, **k: (calls.__setitem__("bwd", calls["bwd"] + 1), real_b(*a, **k))[1])
    torch.manual_seed(31)
    layer = _layers()[kind]()
    with torch.no_grad():
        layer.bias.normal_()
    tol = 2e-2 if bf16 else 2e-5
    x = torch.randn(2, 64, 14, 14, device=DEV)
    gout = torch.randn(2, 64, 14, 14, device=DEV)
    if bf16:
        x, gout = x.bfloat16(), gout.bfloat16()
    x.requires_grad_()
    x64 = x.detach().double().requires_grad_()
    y64, pairs = _reference(kind, layer, x64)                       # before the bias is dropped: the leaves are copies
    if not with_bias:
        layer.bias = None
        y64 = y64 - pairs[-1][2].view(1, -1, 1, 1)
        pairs = pairs[:-1]
    if bf16:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = layer(x)
        assert y.dtype == torch.bfloat16
    else:
        y = layer(x)
    y.backward(gout)
    assert calls == {"save": 1, "bwd": 1}
    y64.backward(gout.double())
    for name, p, l in pairs + [("x", x, x64)]:
        err = _rel(p.grad.reshape(l.grad.shape), l.grad)
        print(f"conv-chain layer {kind} bf16={bf16} bias={with_bias} {name} err={err:.3e}")
        assert err < tol, (name, err)
    assert _rel(y, y64.detach()) < tol
    # frozen factors, trainable input: nothing saved, one data-gradient launch
    for p in layer.parameters():
        p.requires_grad_(False)
    x2 = x.detach().clone().requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        layer(x2).backward(gout)
    assert calls == {"save": 1, "bwd": 2} and _rel(x2.grad, x64.grad) < tol


# ------------------------------------------------------------------------------------------------ refused descriptors
def test_refused_descriptors_launch_nothing():
    from tadmm import _cabi, ops
    case = CASES["1-one-tile"]
    C_, O, r1, r2, hw, k, s, p, dl = case
    x, w1, core, w3, bias, dy, ref = _operands(*case, torch.float32)
    fwd, bwd = _planes(w1, core, w3, torch.float32)
    h = _cabi.Handle.get(torch.cuda.current_device())
    y = torch.full((2, O, 7, 7), SENTINEL, device=DEV)
    h1 = torch.full((2, r1, 7, 7), SENTINEL, device=DEV)
    h2 = torch.full((2, r2, 7, 7), SENTINEL, device=DEV)
    dx = torch.full((2, C_, 7, 7), SENTINEL, device=DEV)

    def desc(planes, src, dst, backward=False, **over):
        d, _, _ = ops._conv_chain_desc(2, C_, 7, 7, O, *planes, None, torch.float32, (3, 3), (1, 1), (1, 1), (1, 1), bwd=backward)
        d.X, d.Y = src.data_ptr(), dst.data_ptr()
        for n, v in over.items():
            setattr(d, n, v)
        return d

    stream = ops._stream(x.device)
    save, back = h.lib.tadmm_ttconv_fused_save, h.lib.tadmm_ttconv_fused_bwd
    P = lambda t: C.c_void_p(t.data_ptr())
    refused = [
        (lambda: save(h.ptr, C.byref(desc(fwd, x, y, Ho=8)), r1, r2, P(h1), P(h2), stream), -1, "output size"),
        (lambda: save(h.ptr, C.byref(desc(fwd, x, y, kh=0)), r1, r2, P(h1), P(h2), stream), -1, "bad geometry"),
        (lambda: save(h.ptr, C.byref(desc(fwd, x, y)), 33, r2, P(h1), P(h2), stream), -1, "true ranks (33, 28)"),
        (lambda: save(h.ptr, C.byref(desc(fwd, x, y)), r1, 0, P(h1), P(h2), stream), -1, "true ranks"),
        (lambda: save(h.ptr, C.byref(desc(fwd, x, y)), r1, r2, None, P(h2), stream), -1, "null intermediate"),
        (lambda: save(h.ptr, C.byref(desc(fwd, x, y)), r1, r2, C.c_void_p(h1.data_ptr() + 2), P(h2), stream), -1, "misaligned"),
        (lambda: save(h.ptr, C.byref(desc(fwd, x, y, R1=288)), r1, r2, P(h1), P(h2), stream), -5, "at most 256"),
        (lambda: save(h.ptr, C.byref(desc(fwd, x, y, W=70, Wo=70)), r1, r2, P(h1), P(h2), stream), -5, "output rows of more than 64"),
        (lambda: back(h.ptr, C.byref(desc(bwd, dy, dx, True)), r1, r2, P(h1), None, stream), -1, "together"),
        (lambda: back(h.ptr, C.byref(desc(bwd, dy, dx, True, X=None)), r1, r2, None, None, stream), -1, "null operand"),
        (lambda: back(h.ptr, C.byref(desc(bwd, dy, dx, True, W=70, Wo=70)), r1, r2, None, None, stream), -5, "input rows of more than 64"),
        (lambda: back(h.ptr, C.byref(desc(bwd, dy, dx, True, w2_plane=512)), r1, r2, None, None, stream), -1, "weight planes"),
    ]
    for i, (call, want, text) in enumerate(refused):
        rc = call()
        assert rc == want, (i, rc, want)
        assert text in h.lib.tadmm_last_error(h.ptr).decode(), (i, h.lib.tadmm_last_error(h.ptr))
    torch.cuda.synchronize()
    for t in (y, h1, h2, dx):
        assert bool((t == SENTINEL).all())
    # B == 0 succeeds with nothing launched, null operands and all
    assert save(h.ptr, C.byref(desc(fwd, x, y, B=0, X=None, Y=None)), r1, r2, None, None, stream) == 0
    assert back(h.ptr, C.byref(desc(bwd, dy, dx, True, B=0, X=None, Y=None)), r1, r2, None, None, stream) == 0
