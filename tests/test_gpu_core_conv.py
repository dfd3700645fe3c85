"""The native k x k core convolution (csrc/coreconv.hip, csrc/wgrad.hip) on the device: forward, data gradient and
weight gradient against float64 `F.conv2d` and its autograd, the autograd Function, and the three factorised layers
forced onto the new path.

Bars (max error over max |reference|): 1e-5 for fp32 Y and dX and for dWc in both dtypes (dWc is float32 and its
products are exact in bf16 mode: the bar of tests/test_gpu_wgrad.py); 3e-2 for bf16 Y and dX against the reference formed
from the bf16-rounded operands (the bar of tests/test_gpu_chain.py)."""
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _rel(y, ref):
    return (y.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _operands(B, r1, r2, hw, k, s, p, dl, dtype, seed=0):
    """Gaussian x, core (scaled by (r1*kh*kw)^-1/2) and dy of `dtype`, and the float64 reference (y, dx, dw) of the
    rounded operands."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    k = _pair(k)
    x = torch.randn(B, r1, *hw, generator=g).to(DEV).to(dtype)
    core = (torch.randn(r2, r1, *k, generator=g) * (r1 * k[0] * k[1]) ** -0.5).to(DEV)
    if dtype == torch.bfloat16:
        core = core.bfloat16().float()                 # the one plane the kernel multiplies with
    x64 = x.double().requires_grad_()
    c64 = core.double().requires_grad_()
    y64 = F.conv2d(x64, c64, None, s, p, dl)
    dy = torch.randn(y64.shape, generator=g).to(DEV).to(dtype)
    dx64, dw64 = torch.autograd.grad(y64, (x64, c64), dy.double())
    return x, core, dy, y64.detach(), dx64, dw64


SHAPES = [
    # B, R1, R2, (H, W), kernel, stride, padding, dilation
    (2, 12, 20, (9, 9), 3, 1, 1, 1),              # ragged ranks; 81-pixel plane: element loads, tiles that end mid-row
    (1, 8, 8, (3, 70), 3, 1, 1, 1),               # two column tiles; the halo crosses the tile boundary
    (2, 16, 24, (9, 8), 3, 2, 1, 1),              # stride 2, (H + 2p - k) % s != 0: the last input row has no output
    (2, 8, 8, (16, 16), 7, 2, 3, 1),              # a 49-tap stem-like kernel
    (2, 24, 24, (6, 6), 5, 1, 2, 1),              # 5 x 5 taps
    (2, 12, 12, (7, 7), 3, 1, 2, 2),              # dilation 2
    (3, 9, 11, (5, 5), 1, 1, 0, 1),               # 1 x 1 core
    (2, 8, 8, (6, 10), (1, 3), 1, (0, 1), 1),     # non-square kernel
    (1, 8, 8, (4, 4), 3, 1, 2, 1),                # output plane larger than the input
]
BIG_RANKS = [(1, 264, 40, (6, 6), 3, 1, 1, 1), (1, 40, 264, (6, 6), 3, 1, 1, 1)]      # rank > 256, either side; fp32 only
CASES = [(s, dt) for s in SHAPES for dt in (torch.float32, torch.bfloat16)] + [(s, torch.float32) for s in BIG_RANKS]


@pytest.mark.parametrize("shape,dtype", CASES, ids=lambda v: str(v).replace(" ", "").replace("torch.", ""))
def test_forward_dgrad_wgrad_match_fp64(shape, dtype):
    from tadmm import ops
    B, r1, r2, hw, k, s, p, dl = shape
    x, core, dy, y64, dx64, dw64 = _operands(B, r1, r2, hw, k, s, p, dl, dtype)
    n = 3 if dtype == torch.float32 else 1
    y = ops.core_conv(x, ops.conv_core_planes(core, n), r2, _pair(k), s, p, dl, memo=False)
    dx = ops.core_conv_dgrad(dy, ops.conv_core_planes(core.permute(1, 0, 2, 3), n), x.shape, _pair(k), s, p, dl, memo=False)
    dw = ops.core_conv_wgrad(dy, x, _pair(k), s, p, dl)
    assert y.shape == y64.shape and y.dtype == dtype and dx.shape == x.shape and dx.dtype == dtype
    assert dw.shape == core.shape and dw.dtype == torch.float32 and dw.is_contiguous()
    ey, ex, ew = _rel(y, y64), _rel(dx, dx64), _rel(dw, dw64)
    print(f"core-conv {shape} {dtype}: Y {ey:.3e} dX {ex:.3e} dWc {ew:.3e}")
    bar = 1e-5 if dtype == torch.float32 else 3e-2
    assert ey < bar, ey
    assert ex < bar, ex
    assert ew < 1e-5, ew


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_exact_weight_gradient_over_several_slices(dtype):
    """X = 0.5, dY = 3: dWc[tap] = 1.5 x the number of in-image source pixels of the tap, exactly."""
    from tadmm import ops
    x = torch.full((4, 1, 32, 32), 0.5, device=DEV, dtype=dtype)
    dy = torch.full((4, 1, 32, 32), 3.0, device=DEV, dtype=dtype)
    nbytes, slices = ops.core_conv_wgrad_plan(dy, x, (3, 3), 1, 1, 1)
    assert slices > 1 and nbytes > 0
    dw = ops.core_conv_wgrad(dy, x, (3, 3), 1, 1, 1)
    cnt = torch.tensor([[32 - abs(ky - 1), 32 - abs(kx - 1)] for ky in range(3) for kx in range(3)], dtype=torch.float64)
    want = (1.5 * 4 * cnt[:, 0] * cnt[:, 1]).reshape(1, 1, 3, 3)
    assert torch.equal(dw.double().cpu(), want), (dw, want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_weight_gradient_is_bitwise_deterministic_and_ignores_the_workspace(dtype):
    from tadmm import ops
    x, core, dy, *_ = _operands(4, 12, 20, (32, 32), 3, 1, 1, 1, dtype, seed=5)
    nbytes, slices = ops.core_conv_wgrad_plan(dy, x, (3, 3), 1, 1, 1)
    assert slices > 1
    first = ops.core_conv_wgrad(dy, x, (3, 3), 1, 1, 1)
    ws = torch.full((nbytes // 4,), float("nan"), device=DEV).view(torch.uint8)
    second = ops.core_conv_wgrad(dy, x, (3, 3), 1, 1, 1, workspace=ws)
    assert torch.equal(first, second)
    assert torch.isfinite(second).all()


def _offset_view(t):
    """A contiguous view of t's values at element offset 1 of a NaN-filled flat buffer."""
    flat = torch.full((t.numel() + 16,), float("nan"), device=t.device, dtype=t.dtype)
    flat[1:1 + t.numel()] = t.reshape(-1)
    v = flat[1:1 + t.numel()].view(t.shape)
    assert v.data_ptr() == flat.data_ptr() + t.element_size() and v.is_contiguous()
    return v


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_unaligned_operands_give_the_same_bits(dtype):
    from tadmm import ops
    x, core, dy, *_ = _operands(2, 12, 20, (9, 9), 3, 1, 1, 1, dtype, seed=7)
    n = 3 if dtype == torch.float32 else 1
    wp, wpt = ops.conv_core_planes(core, n), ops.conv_core_planes(core.permute(1, 0, 2, 3), n)
    xu, dyu = _offset_view(x), _offset_view(dy)
    assert torch.equal(ops.core_conv(x, wp, 20, (3, 3), 1, 1, 1, memo=False), ops.core_conv(xu, wp, 20, (3, 3), 1, 1, 1, memo=False))
    assert torch.equal(ops.core_conv_dgrad(dy, wpt, x.shape, (3, 3), 1, 1, 1, memo=False),
                       ops.core_conv_dgrad(dyu, wpt, x.shape, (3, 3), 1, 1, 1, memo=False))
    assert torch.equal(ops.core_conv_wgrad(dy, x, (3, 3), 1, 1, 1), ops.core_conv_wgrad(dyu, xu, (3, 3), 1, 1, 1))


def test_empty_batch():
    from tadmm import ops
    x = torch.zeros(0, 12, 9, 9, device=DEV)
    core = torch.randn(20, 12, 3, 3, device=DEV)
    y = ops.core_conv(x, ops.conv_core_planes(core, 3), 20, (3, 3), 2, 1, 1, memo=False)
    assert y.shape == (0, 20, 5, 5)
    dx = ops.core_conv_dgrad(y, ops.conv_core_planes(core.permute(1, 0, 2, 3), 3), x.shape, (3, 3), 2, 1, 1, memo=False)
    assert dx.shape == (0, 12, 9, 9)
    dw = ops.core_conv_wgrad(y, x, (3, 3), 2, 1, 1)
    assert dw.shape == (20, 12, 3, 3) and dw.abs().max().item() == 0.0


# ------------------------------------------------------------------------------------------------ autograd
def test_autograd_matches_fp64_on_the_stride_2_shape():
    from tadmm import functional as HF
    x, core, dy, y64, dx64, dw64 = _operands(2, 16, 24, (9, 8), 3, 2, 1, 1, torch.float32, seed=9)
    xg, cg = x.clone().requires_grad_(), core.clone().requires_grad_()
    y = HF.core_conv(xg, cg, 2, 1, 1)
    dx, dw = torch.autograd.grad(y, (xg, cg), dy)
    assert _rel(y, y64) < 1e-5 and _rel(dx, dx64) < 1e-5 and _rel(dw, dw64) < 1e-5


def test_backward_computes_only_what_is_asked_for(monkeypatch):
    from tadmm import functional as HF
    from tadmm import ops
    x, core, dy, y64, dx64, dw64 = _operands(2, 16, 24, (9, 8), 3, 2, 1, 1, torch.float32, seed=10)
    calls = {"dgrad": 0, "wgrad": 0}
    real_d, real_w = ops.core_conv_dgrad, ops.core_conv_wgrad
    monkeypatch.setattr(ops, "core_conv_dgrad", lambda *a, **k: (calls.__setitem__("dgrad", calls["dgrad"] + 1), real_d(*a, **k))[1])
    monkeypatch.setattr(ops, "core_conv_wgrad", lambda *a, **k: (calls.__setitem__("wgrad", calls["wgrad"] + 1), real_w(*a, **k))[1])
    cg = core.clone().requires_grad_()
    HF.core_conv(x, cg, 2, 1, 1).backward(dy)                     # x wants no gradient: no data-gradient launch
    assert calls == {"dgrad": 0, "wgrad": 1} and _rel(cg.grad, dw64) < 1e-5
    xg = x.clone().requires_grad_()
    HF.core_conv(xg, core, 2, 1, 1).backward(dy)                  # frozen core, trainable x: dX only
    assert calls == {"dgrad": 1, "wgrad": 1} and _rel(xg.grad, dx64) < 1e-5


def test_autocast_weight_gradient_takes_the_parameters_dtype():
    from tadmm import functional as HF
    x, core, dy, y64, dx64, dw64 = _operands(2, 16, 24, (9, 8), 3, 2, 1, 1, torch.bfloat16, seed=11)
    cg = core.clone().requires_grad_()                              # a float32 parameter under bf16 activations
    y = HF.core_conv(x, cg, 2, 1, 1)
    assert y.dtype == torch.bfloat16
    y.backward(dy)
    assert cg.grad.dtype == torch.float32 and _rel(cg.grad, dw64) < 1e-5


# ------------------------------------------------------------------------------------------------ layers
class _HP:
    pass


def _raising_functional():
    def conv2d(*a, **k):
        raise AssertionError("the device library's conv2d was called")
    ns = types.SimpleNamespace(**{n: getattr(F, n) for n in dir(F) if not n.startswith("__")})
    ns.conv2d = conv2d
    return ns


def _recover64(cores):
    w = cores[0].reshape(-1, cores[0].shape[-1])
    for c in cores[1:]:
        w = w.reshape(-1, c.shape[0]) @ c.reshape(c.shape[0], -1)
    return w


def _layers():
    from tadmm import tk_layers, tt_layers
    hp = _HP()
    hp.tt_shapes = {"c.weight": [8, 8, 9, 8, 8]}
    hp.ranks = {"c.weight": [1, 8, 40, 40, 8, 1]}
    hk = _HP()
    hk.ranks = {"k.weight": [25, 23]}
    return {
        "ttm": lambda: tt_layers.TTConv2dM(64, 64, 3, padding=1, bias=True, hp_dict=hp, name="c.weight").to(DEV),
        "tkc": lambda: tk_layers.TKConv2dC(64, 64, 3, padding=1, bias=True, hp_dict=hk, name="k.weight").to(DEV),
        "tkm": lambda: tk_layers.TKConv2dM(64, 64, 3, padding=1, bias=True, hp_dict=hk, name="k.weight").to(DEV),
    }


def _reference(kind, layer, x64):
    """float64 composition 1x1 -> k x k -> 1x1 + bias of the layer's parameters; returns (y64, [(name, param, leaf)])."""
    def leaf(p):
        return p.detach().double().requires_grad_()
    if kind == "ttm":
        ins, outs = [leaf(c) for c in layer.in_tt_cores], [leaf(c) for c in layer.out_tt_cores]
        core, b = leaf(layer.core_kernel), leaf(layer.bias)
        w1 = _recover64(ins).reshape(layer.in_tt_ranks[0], 64)
        w3 = _recover64(outs).reshape(64, layer.out_tt_ranks[-1])
        pairs = ([(f"in_tt_cores[{i}]", p, l) for i, (p, l) in enumerate(zip(layer.in_tt_cores, ins))]
                 + [(f"out_tt_cores[{i}]", p, l) for i, (p, l) in enumerate(zip(layer.out_tt_cores, outs))]
                 + [("core_kernel", layer.core_kernel, core), ("bias", layer.bias, b)])
    else:
        names = ("first_kernel", "core_kernel", "last_kernel", "bias") if kind == "tkc" else \
            ("first_factor", "core_kernel", "last_factor", "bias")
        leaves = [leaf(getattr(layer, n)) for n in names]
        w1, core, w3, b = leaves[0].reshape(layer.in_rank, 64), leaves[1], leaves[2].reshape(64, layer.out_rank), leaves[3]
        pairs = [(n, getattr(layer, n), l) for n, l in zip(names, leaves)]
    y64 = F.conv2d(F.conv2d(F.conv2d(x64, w1[:, :, None, None]), core, padding=1), w3[:, :, None, None], b)
    return y64, pairs


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("kind", ["ttm", "tkc", "tkm"])
def test_layers_forced_onto_the_native_core_convolution(kind, bf16, monkeypatch):
    from tadmm import functional as HF, ops, tt_layers
    monkeypatch.setattr(ops, "core_conv_pays", lambda *a, **k: True)
    monkeypatch.setattr(HF, "F", _raising_functional())            # the fallback conv2d of `functional.conv_stages`
    monkeypatch.setattr(tt_layers, "F", _raising_functional())     # (tk_layers no longer imports it)
    torch.manual_seed(21)
    layer = _layers()[kind]()
    with torch.no_grad():
        layer.bias.normal_()
    tol = 2e-2 if bf16 else 2e-5
    x = torch.randn(2, 64, 14, 14, device=DEV)
    gout = torch.randn(2, 64, 14, 14, device=DEV)
    if bf16:
        x, gout = x.bfloat16(), gout.bfloat16()
    x.requires_grad_()
    if bf16:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = layer(x)
        assert y.dtype == torch.bfloat16
    else:
        y = layer(x)
    y.backward(gout)
    x64 = x.detach().double().requires_grad_()
    y64, pairs = _reference(kind, layer, x64)
    y64.backward(gout.double())
    for name, p, l in pairs + [("x", x, x64)]:
        err = _rel(p.grad.reshape(l.grad.shape), l.grad)
        print(f"core-conv layer {kind} bf16={bf16} {name} err={err:.3e}")
        assert err < tol, (name, err)
    assert _rel(y, y64.detach()) < tol
    # inference on rows of 70 pixels: the one-launch kernel is ineligible, the native core convolution serves
    wide = torch.randn(1, 64, 3, 70, device=DEV)
    if bf16:
        wide = wide.bfloat16()
    calls = []
    real = ops.core_conv
    monkeypatch.setattr(ops, "core_conv", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        yw = layer(wide)
        yw2 = layer(wide)                                           # the cached planes
    assert len(calls) == 2 and torch.equal(yw, yw2)
    yw64, _ = _reference(kind, layer, wide.double())
    assert _rel(yw, yw64.detach()) < tol
