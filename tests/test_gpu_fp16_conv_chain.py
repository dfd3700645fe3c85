"""The one-launch factorised convolution (csrc/convchain.hip, `tadmm_ttconv_fused`) on float16 images: one binary16
plane per weight, H1 and H2 rounded to binary16 in LDS, fp32 accumulation.  Reference: the float64 composition
1x1 -> k x k -> 1x1 + bias of the rounded operands; bound: the three-stage bound of tests/_fp16_ref.py (u = 2^-11),
elementwise.  The saving forward and the data gradient refuse float16."""
import functools

import pytest
import torch

from _fp16_ref import bits, conv_bound, report

pytestmark = pytest.mark.gpu
F16 = torch.float16
RAGGED = (24, 40, 20, 24)                               # C, O, r1, r2: ranks that need padding to 32
# (C, O, r1, r2, (H, W), k, stride, padding, dilation, B)
CASES = {
    "7x7-one-tile": (*RAGGED, (7, 7), 3, 1, 1, 1, 2),
    "14x14-stride2-to-7x7": (*RAGGED, (14, 14), 3, 2, 1, 1, 2),
    "28x28-row-tiles": (*RAGGED, (28, 28), 3, 1, 1, 1, 2),
    "8x8-3x3-stride2-pad0": (*RAGGED, (8, 8), 3, 2, 0, 1, 2),
    "9x9-5x5-dilation2": (*RAGGED, (9, 9), 5, 1, 2, 2, 2),
    "6x10-1x3": (*RAGGED, (6, 10), (1, 3), 1, (0, 1), 1, 2),
    "width-64": (8, 8, 12, 20, (2, 64), 3, 1, 1, 1, 2),
    "ranks-above-128": (40, 48, 136, 72, (7, 7), 3, 1, 1, 1, 2),      # four feature tiles per wave
}


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Operands, planes and the float64 reference with its bound: built once, never modified."""
    from tadmm import ops
    C_, O, r1, r2, hw, k, s, p, dl, B = CASES[name]
    k, s, p, dl = _pair(k), _pair(s), _pair(p), _pair(dl)
    g = torch.Generator(device="cpu").manual_seed(len(name))
    x = torch.randn(B, C_, *hw, generator=g).cuda().half()
    w1 = (torch.randn(r1, C_, generator=g) * C_ ** -0.5).cuda()
    core = (torch.randn(r2, r1, *k, generator=g) * (r1 * k[0] * k[1]) ** -0.5).cuda()
    w3 = (torch.randn(O, r2, generator=g) * r2 ** -0.5).cuda()
    bias = torch.randn(O, generator=g).cuda()
    planes = (ops.weight_planes(w1, 1, pad_rows=32, dtype=F16), ops.conv_core_planes(core, 1, dtype=F16),
              ops.weight_planes(w3, 1, dtype=F16))
    ref, bound = conv_bound(x, w1.half(), core.half(), w3.half(), bias, s, p, dl, F16)
    return x, planes, bias, (O, k, s, p, dl), ref, bound


@pytest.mark.parametrize("name", list(CASES))
def test_conv_chain_matches_fp64(name):
    from tadmm import ops
    x, planes, bias, (O, k, s, p, dl), ref, bound = _case(name)
    assert ops.conv_chain_fits(x, planes[0].shape[1] * 16, planes[1].shape[1] * 16, k, s, p, dl)
    y = ops.conv_chain(x, *planes, bias, O, k, s, p, dl)
    assert y.dtype == F16 and y.shape == ref.shape
    report(f"conv chain {name}", y, ref, bound)
    # deterministic, and `out=` writes the same bits
    out = torch.full(ref.shape, 7.0, dtype=F16, device="cuda")
    y2 = ops.conv_chain(x, *planes, bias, O, k, s, p, dl, out=out)
    assert y2 is out and torch.equal(bits(y2), bits(y))


def test_no_bias():
    from tadmm import ops
    x, planes, bias, (O, k, s, p, dl), ref, bound = _case("7x7-one-tile")
    y0 = ops.conv_chain(x, *planes, None, O, k, s, p, dl)
    report("conv chain no bias", y0, ref - bias.double().view(1, -1, 1, 1), bound)


def test_refusals_launch_nothing():
    from tadmm import ops
    from tadmm._cabi import TadmmError
    x, planes, bias, (O, k, s, p, dl), ref, _ = _case("7x7-one-tile")
    out = torch.full(ref.shape, 7.0, dtype=F16, device="cuda")
    bf_planes = tuple(t.view(torch.bfloat16) for t in planes)           # the same words read as the other 16-bit type
    with pytest.raises(TadmmError):                                       # bf16 planes under float16 images
        ops.conv_chain(x, *bf_planes, bias, O, k, s, p, dl, out=out)
    with pytest.raises(TadmmError):                                       # one plane of the wrong type is enough
        ops.conv_chain(x, planes[0], bf_planes[1], planes[2], bias, O, k, s, p, dl, out=out)
    with pytest.raises(TadmmError):                                       # float16 planes under bfloat16 images
        ops.conv_chain(x.bfloat16(), *planes, bias, O, k, s, p, dl)
    B, _, H, W = x.shape
    r1, r2 = 20, 24
    h1 = torch.full((B, r1, H, W), 7.0, dtype=F16, device="cuda")
    h2 = torch.full((B, r2, *ref.shape[2:]), 7.0, dtype=F16, device="cuda")
    with pytest.raises(TadmmError):                                       # nothing is saved in float16
        ops.conv_chain_save(x, *planes, bias, O, r1, r2, k, s, p, dl, out=(out, h1, h2))
    with pytest.raises(TadmmError):                                       # and there is no float16 data gradient
        ops.conv_chain_bwd(ref.half(), *planes, tuple(x.shape), r1, r2, k, s, p, dl)
    torch.cuda.synchronize()
    for t in (out, h1, h2):
        assert bool((t == 7.0).all())
    # the library itself refuses the two training entries
    import ctypes as C
    from tadmm import _cabi
    d, _, _ = ops._conv_chain_desc(B, x.shape[1], H, W, O, *planes, bias, F16, k, s, p, dl)
    d.X, d.Y = x.data_ptr(), out.data_ptr()
    h = ops.Handle.get(torch.cuda.current_device())
    assert d.dtype == _cabi.CHAIN_F16
    assert h.lib.tadmm_ttconv_fused_save(h.ptr, C.byref(d), r1, r2, h1.data_ptr(), h2.data_ptr(), 0) == -1
    assert h.lib.tadmm_ttconv_fused_bwd(h.ptr, C.byref(d), r1, r2, None, None, 0) == -1
    torch.cuda.synchronize()
    for t in (out, h1, h2):
        assert bool((t == 7.0).all())
