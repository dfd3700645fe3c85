"""The factorised layers on float16 activations under `torch.no_grad()` -- what the reference's `evaluate()` under
autocast hands them: the result is float16, it comes from the native one-plane kernels (recorded at `ops.chain_fused`,
`ops.chain_single`, `ops.svd_conv`, `ops.conv_chain`), and it lies inside the derived bound of tests/_fp16_ref.py
against the float64 composition of the factors rounded to binary16 (TT layers enter through their contracted factors:
those are what the kernels multiply).  One module serves bfloat16, float16 and float32 callers from separate caches,
and grad mode keeps the per-core float32 route."""
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from _fp16_ref import bits, conv_bound, image_rows, linear_bound, report

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


class _HP:
    pass


def _hp(**kw):
    hp = _HP()
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def _unit_scale(cores_in, cores_out, factors, k_in, k_out):
    """Rescale the first core of each chain so that the contracted factors have fan-in^-1/2 entries (Gaussian-sized
    activations all the way: nothing near binary16's overflow or its subnormals)."""
    with torch.no_grad():
        w_in, w_out = factors()
        cores_in[0].mul_(1.0 / (w_in.std().item() * k_in ** 0.5))
        cores_out[0].mul_(1.0 / (w_out.std().item() * k_out ** 0.5))


def _build(kind):
    """(layer, float32 input, kind of reference).  Small shapes; every layer has a bias with Gaussian entries."""
    from tadmm import svd_layers, tk_layers, tt_layers
    torch.manual_seed(7 * len(kind))
    g = torch.Generator(device="cpu").manual_seed(len(kind))
    if kind == "ttlinear":
        hp = _hp(tt_shapes={"qkv.weight": [36, 32, 16, 24]}, ranks={"qkv.weight": [1, 25, 256, 18, 1]})
        layer = tt_layers.TTLinearM(384, 1152, bias=True, hp_dict=hp, name="qkv.weight").to(DEV)
        q = layer.out_tt_order
        _unit_scale(layer.tt_cores[q:], layer.tt_cores[:q], layer._factors, 384, 256)
        x = torch.randn(2, 197, 384, generator=g)
    elif kind == "tklinear":
        layer = tk_layers.TKLinearM(64, 48, bias=True, hp_dict=_hp(ranks={"w": [24, 20]}), name="w").to(DEV)
        with torch.no_grad():
            layer.first_factor.normal_(0, 64 ** -0.5), layer.core_tensor.normal_(0, 20 ** -0.5), layer.last_factor.normal_(0, 24 ** -0.5)
        x = torch.randn(70, 64, generator=g)
    elif kind in ("ttconv", "ttconv-wide"):
        hp = _hp(tt_shapes={"c.weight": [8, 8, 9, 8, 8]}, ranks={"c.weight": [1, 8, 40, 40, 8, 1]})
        layer = tt_layers.TTConv2dM(64, 64, 3, padding=1, bias=True, hp_dict=hp, name="c.weight").to(DEV)
        _unit_scale(layer.in_tt_cores, layer.out_tt_cores, layer._factors, 64, 40)
        with torch.no_grad():
            layer.core_kernel.normal_(0, (40 * 9) ** -0.5)
        x = torch.randn(2, 64, 14, 14, generator=g) if kind == "ttconv" else torch.randn(1, 64, 5, 72, generator=g)
    elif kind in ("tkconv-c", "tkconv-m"):
        cls = tk_layers.TKConv2dC if kind == "tkconv-c" else tk_layers.TKConv2dM
        layer = cls(64, 64, 3, padding=1, bias=True, hp_dict=_hp(ranks={"k.weight": [25, 23]}), name="k.weight").to(DEV)
        x = torch.randn(2, 64, 14, 14, generator=g)
    else:
        cls = svd_layers.SVDConv2dC if kind == "svdconv-c" else svd_layers.SVDConv2dM
        layer = cls(48, 36, 1, bias=True, hp_dict=_hp(ranks={"s.weight": 20}), name="s.weight").to(DEV)
        x = torch.randn(3, 48, 7, 7, generator=g)
    with torch.no_grad():
        layer.bias.normal_()
    return layer.eval(), x.to(DEV)


KINDS = ["ttlinear", "tklinear", "ttconv", "ttconv-wide", "tkconv-c", "tkconv-m", "svdconv-c", "svdconv-m"]
# the native entries a float16 inference call must reach
ENTRIES = {"ttlinear": ["chain_fused"], "tklinear": ["chain_fused"], "ttconv": ["conv_chain"],
           "ttconv-wide": ["chain_single", "chain_single"], "tkconv-c": ["conv_chain"], "tkconv-m": ["conv_chain"],
           "svdconv-c": ["svd_conv"], "svdconv-m": ["svd_conv"]}


def _factors32(kind, layer):
    """The float32 factors the layer's kernels pack (contracted where the layer contracts), and the bias."""
    from tadmm import functional as HF
    with torch.no_grad():
        if kind == "ttlinear":
            return list(layer._factors()), layer.bias
        if kind == "tklinear":
            return [HF.mm(layer.core_tensor, layer.first_factor), layer.last_factor.detach()], layer.bias
        if kind.startswith("ttconv"):
            w_in, w_out = layer._factors()
            return [w_in, layer.core_kernel.detach(), w_out], layer.bias
        if kind == "tkconv-c":
            return [layer.first_kernel.reshape(layer.in_rank, -1), layer.core_kernel.detach(),
                    layer.last_kernel.reshape(-1, layer.out_rank)], layer.bias
        if kind == "tkconv-m":
            return [layer.first_factor.detach(), layer.core_kernel.detach(), layer.last_factor.detach()], layer.bias
        if kind == "svdconv-c":
            return [layer.left_kernel.reshape(layer.rank, -1), layer.right_kernel.reshape(-1, layer.rank)], layer.bias
        return [layer.left_factor.detach(), layer.right_factor.detach()], layer.bias


def _ref_and_bound(kind, layer, x, dtype):
    """float64 composition of the factors rounded to `dtype`, the bound for that dtype, and y -> comparable rows."""
    ws, bias = _factors32(kind, layer)
    ws = [w.to(dtype) for w in ws]
    if len(ws) == 3:
        ref, bound = conv_bound(x, *ws, bias, layer.stride, layer.padding, layer.dilation, dtype)
        return ref, bound, lambda y: y
    if x.dim() == 4:
        ref, bound = linear_bound(image_rows(x), ws, bias, dtype)
        return ref, bound, image_rows
    ref, bound = linear_bound(x.reshape(-1, x.shape[-1]), ws, bias, dtype)
    return ref, bound, lambda y: y.reshape(-1, y.shape[-1])


def _record(monkeypatch):
    from tadmm import ops
    calls = []
    for name in ("chain_fused", "chain_single", "svd_conv", "conv_chain"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **k: (calls.append((_n, a[0].dtype)), _r(*a, **k))[1])
    return calls


@pytest.mark.parametrize("kind", KINDS)
def test_float16_inference_runs_the_native_kernels(kind, monkeypatch):
    layer, x = _build(kind)
    calls = _record(monkeypatch)
    with torch.no_grad():
        y = layer(x.half())
    assert y.dtype == F16
    assert calls == [(n, F16) for n in ENTRIES[kind]], calls
    ref, bound, rows = _ref_and_bound(kind, layer, x.half(), F16)
    assert rows(y).shape == ref.shape
    report(f"layer {kind}", rows(y), ref, bound)


@pytest.mark.parametrize("kind", ["ttconv", "tkconv-c", "svdconv-m"])
def test_evaluate_pattern_under_autocast(kind, monkeypatch):
    """`evaluate()` of the reference: no_grad + autocast(float16) around a model fed float32 images."""
    layer, x = _build(kind)
    torch.manual_seed(3)
    cin = x.shape[1]
    model = nn.Sequential(nn.Conv2d(3, cin, 3, padding=1), layer).to(DEV).eval()
    seen = []
    layer.register_forward_pre_hook(lambda m, args: seen.append(args[0].dtype))
    calls = _record(monkeypatch)
    img = torch.randn(2, 3, *x.shape[2:], device=DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=F16):
        y = model(img)
        mid = model[0](img)
    assert img.dtype == F32 and seen == [F16] and mid.dtype == F16
    assert y.dtype == F16 and calls == [(n, F16) for n in ENTRIES[kind]], calls
    ref, bound, rows = _ref_and_bound(kind, layer, mid, F16)
    report(f"evaluate {kind}", rows(y), ref, bound)


@pytest.mark.parametrize("kind", ["ttlinear", "tklinear", "ttconv", "tkconv-c", "tkconv-m", "svdconv-c", "svdconv-m"])
def test_one_module_keeps_its_dtypes_apart(kind):
    layer, x = _build(kind)
    fresh = copy.deepcopy(layer)                        # same parameters, no cache yet
    rows = None
    with torch.no_grad():
        yb = layer(x.bfloat16())
        yh = layer(x.half())
        yf = layer(x)
        yh2 = layer(x.half())
        yb_fresh = fresh(x.bfloat16())
    assert (yb.dtype, yh.dtype, yf.dtype, yh2.dtype) == (BF16, F16, F32, F16)
    for y, dt in ((yb, BF16), (yh, F16), (yh2, F16)):
        ref, bound, rows = _ref_and_bound(kind, layer, x.to(dt), dt)
        report(f"shared module {kind} {dt}", rows(y), ref, bound)
    # float32: three planes, fp32-GEMM accuracy (2e-5 of max|ref|: the bar tests/test_gpu_core_conv.py holds the float32
    # layers to)
    ws, bias = _factors32(kind, layer)
    if len(ws) == 3:
        r = F.conv2d(F.conv2d(F.conv2d(x.double(), ws[0].double()[:, :, None, None]), ws[1].double(), None, layer.stride,
                              layer.padding, layer.dilation), ws[2].double()[:, :, None, None], bias.double())
        err = (yf.double() - r).abs().max().item() / r.abs().max().item()
    else:
        xr = image_rows(x) if x.dim() == 4 else x.reshape(-1, x.shape[-1])
        r = (xr.double() @ ws[0].double().t()) @ ws[1].double().t() + bias.double()
        err = (rows(yf).double() - r).abs().max().item() / r.abs().max().item()
    print(f"fp16 shared module {kind} float32: max err / max|ref| {err:.3e}")
    assert err < 2e-5, err
    assert torch.equal(bits(yh2), bits(yh))
    assert torch.equal(bits(yb), bits(yb_fresh))
    assert not torch.equal(yh.float(), yb.float())      # the two 16-bit results are different numbers


def test_grad_mode_keeps_the_per_core_float32_route(monkeypatch):
    calls = _record(monkeypatch)
    lin, x = _build("ttlinear")
    assert all(p.requires_grad for p in lin.parameters()) and torch.is_grad_enabled()
    y = lin(x.half())
    assert y.dtype == F32 and torch.equal(y, lin._forward_chain(x.half()))
    conv, xc = _build("ttconv")
    yc = conv(xc.half())
    assert yc.dtype == F32 and torch.equal(yc, conv._chains(xc.half())[0])
    tk, xt = _build("tklinear")
    from tadmm import functional as HF
    yt = tk(xt.half())
    want = HF.linear(HF.linear(HF.linear(xt.half(), tk.first_factor), tk.core_tensor), tk.last_factor, tk.bias)
    assert yt.dtype == F32 and torch.equal(yt, want)
    assert calls == []
    # an input that wants a gradient is grad mode too, whatever the parameters say
    for p in lin.parameters():
        p.requires_grad_(False)
    xg = x.half().requires_grad_()
    assert lin(xg).dtype == F32 and calls == []
    # ... and with nothing left that wants one, the same module takes the kernel
    assert lin(x.half()).dtype == F16 and calls == [("chain_fused", F16)]
