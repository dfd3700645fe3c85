"""The chain kernels (csrc/chain.hip) on float16 activations through `tadmm.ops`: TADMM_CHAIN_F16, one binary16 weight
plane, fp32 accumulation, round-to-nearest-even results that overflow to inf.

1. Rounding, bit for bit: with W = identity the fp32 accumulator is exactly x, so y must be `(x.float() + bias).half()`.
2. The fused chain, the single products and the 1x1 chain on images against float64 products of the rounded operands,
   inside the derived elementwise bound of tests/_fp16_ref.py (u = 2^-11).
3. Refusals before any launch: planes of the other 16-bit type, three binary16 planes, misaligned token rows."""
import ctypes as C

import pytest
import torch

from _fp16_ref import bits, image_rows, linear_bound, report, rows_image

pytestmark = pytest.mark.gpu
F16 = torch.float16


def _ops():
    from tadmm import ops
    return ops


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


# ------------------------------------------------------------------ 1. rounding
def _identity_case(x):
    ops = _ops()
    g = _gen(11)
    bias = torch.randn(48, generator=g)
    bias[5] = 7e4                                       # beyond 65504: the column must be +inf, not 65504
    bias = bias.cuda()
    wp = ops.weight_planes(torch.eye(48, device="cuda"), 1, dtype=F16)
    assert wp.dtype == F16 and wp.shape == (1, 3, 2, 64, 8)          # 48 rows in 3 tiles, 48 columns padded to 64
    return wp, bias


def test_rounding_is_nearest_even_with_overflow_to_inf_on_token_rows():
    ops = _ops()
    x = (torch.randn(50, 48, generator=_gen(1)) * 3).cuda().half()
    wp, bias = _identity_case(x)
    y = ops.chain_single(x, wp, bias, 48)
    want = (x.float() + bias).half()
    assert y.dtype == F16 and y.shape == (50, 48)
    assert torch.isinf(want[:, 5]).all() and (want[:, 5] > 0).all()
    assert torch.equal(bits(y), bits(want))
    # no bias: the identity returns x itself
    assert torch.equal(bits(ops.chain_single(x, wp, None, 48)), bits(x))


def test_rounding_is_nearest_even_with_overflow_to_inf_on_images():
    ops = _ops()
    x = (torch.randn(3, 48, 7, 7, generator=_gen(2)) * 3).cuda().half()     # 49 pixels: scalar loads, straddled tiles
    wp, bias = _identity_case(x)
    y = ops.chain_single(x, wp, bias, 48, image_out=True)
    want = (x.float() + bias.view(1, -1, 1, 1)).half()
    assert y.dtype == F16 and y.shape == x.shape
    assert torch.isinf(want[:, 5]).all()
    assert torch.equal(bits(y), bits(want))


# ------------------------------------------------------------------ 2. against float64
def _factors(g, kin, r, nout):
    win = (torch.randn(r, kin, generator=g) / kin ** 0.5).cuda()
    wout = (torch.randn(nout, r, generator=g) / r ** 0.5).cuda()
    bias = torch.randn(nout, generator=g).cuda()
    return win, wout, bias


@pytest.mark.parametrize("T,kin,r,nout,tile", [
    (77, 64, 32, 24, 0),
    (197, 384, 96, 384, 0),          # ragged token tile, middle rank not a multiple of 64
    (50, 72, 20, 40, 0),             # Kin, R, Nout all need padding
    (1, 1536, 256, 384, 0),          # one token, long K
    (130, 384, 256, 1152, 32),       # 32-token tiles, five of them
])
def test_fused_chain(T, kin, r, nout, tile):
    ops = _ops()
    g = _gen(T + kin)
    x = torch.randn(T, kin, generator=g).cuda().half()
    win, wout, bias = _factors(g, kin, r, nout)
    wp_in = ops.weight_planes(win, 1, pad_rows=64, dtype=F16)
    wp_out = ops.weight_planes(wout, 1, pad_cols=64, dtype=F16)
    assert wp_in.dtype == F16 and torch.equal(ops.unpack_planes(wp_in)[0, :r, :kin], win.half())
    y = ops.chain_fused(x, wp_in, wp_out, bias, nout, tile_tokens=tile)
    assert y.dtype == F16 and y.shape == (T, nout)
    ref, bound = linear_bound(x, [ops.unpack_planes(wp_in)[0, :r, :kin], ops.unpack_planes(wp_out)[0, :nout, :r]], bias, F16)
    report(f"fused {T}x{kin}->{r}->{nout} tile {tile}", y, ref, bound)
    # the data-gradient entry is the same kernel
    y2 = ops.chain_fused(x, wp_in, wp_out, bias, nout, entry="tadmm_ttlinear_bwd", tile_tokens=tile)
    assert torch.equal(bits(y2), bits(y))


@pytest.mark.parametrize("T,kin,n", [(77, 64, 24), (300, 96, 520)])
def test_single_product_rows_to_rows(T, kin, n):
    ops = _ops()
    g = _gen(T + n)
    x = torch.randn(T, kin, generator=g).cuda().half()
    w = (torch.randn(n, kin, generator=g) / kin ** 0.5).cuda()
    bias = torch.randn(n, generator=g).cuda()
    wp = ops.weight_planes(w, 1, dtype=F16)
    for entry in ("tadmm_ttconv_chain_in", "tadmm_tucker_1x1"):
        y = ops.chain_single(x, wp, bias, n, entry=entry)
        assert y.dtype == F16 and y.shape == (T, n)
        ref, bound = linear_bound(x, [ops.unpack_planes(wp)[0, :n, :kin]], bias, F16)
        report(f"single rows {T}x{kin}->{n} {entry}", y, ref, bound)


@pytest.mark.parametrize("B,c,hw,n", [
    (4, 64, (14, 14), 40),           # vectorised image loads and stores
    (2, 512, (7, 7), 300),           # more than 256 output features: two feature blocks; 49 pixels: scalar loads
])
def test_single_product_images_to_images(B, c, hw, n):
    ops = _ops()
    g = _gen(B * c + n)
    x = torch.randn(B, c, *hw, generator=g).cuda().half()
    w = (torch.randn(n, c, generator=g) / c ** 0.5).cuda()
    bias = torch.randn(n, generator=g).cuda()
    wp = ops.weight_planes(w, 1, dtype=F16)
    y = ops.chain_single(x, wp, bias, n, entry="tadmm_ttconv_chain_out", image_out=True)
    assert y.dtype == F16 and y.shape == (B, n, *hw)
    ref, bound = linear_bound(image_rows(x), [ops.unpack_planes(wp)[0, :n, :c]], bias, F16)
    report(f"single image {B}x{c}x{hw}->{n}", image_rows(y), ref, bound)


@pytest.mark.parametrize("B,c,hw,r,n", [(3, 48, (7, 7), 20, 36), (4, 64, (14, 14), 96, 80)])
def test_1x1_chain_on_images(B, c, hw, r, n):
    ops = _ops()
    g = _gen(B + c + r)
    x = torch.randn(B, c, *hw, generator=g).cuda().half()
    win, wout, bias = _factors(g, c, r, n)
    wp_in = ops.weight_planes(win, 1, pad_rows=64, dtype=F16)
    wp_out = ops.weight_planes(wout, 1, pad_cols=64, dtype=F16)
    y = ops.svd_conv(x, wp_in, wp_out, bias, n)
    assert y.dtype == F16 and y.shape == (B, n, *hw)
    ref, bound = linear_bound(image_rows(x), [ops.unpack_planes(wp_in)[0, :r, :c], ops.unpack_planes(wp_out)[0, :n, :r]], bias, F16)
    report(f"1x1 chain {B}x{c}x{hw}->{r}->{n}", image_rows(y), ref, bound)
    y2 = ops.svd_conv(x, wp_in, wp_out, bias, n, entry="tadmm_svdconv_bwd")
    assert torch.equal(bits(y2), bits(y))


# ------------------------------------------------------------------ 3. refusals
def test_refusals_launch_nothing():
    from tadmm import _cabi
    from tadmm._cabi import TadmmError
    ops = _ops()
    g = _gen(3)
    x = torch.randn(40, 64, generator=g).cuda()
    win, wout, bias = _factors(g, 64, 32, 24)
    bf_in, bf_out = ops.weight_planes(win, 1, pad_rows=64), ops.weight_planes(wout, 1, pad_cols=64)
    hf_in, hf_out = (ops.weight_planes(win, 1, pad_rows=64, dtype=F16), ops.weight_planes(wout, 1, pad_cols=64, dtype=F16))
    img = torch.randn(2, 64, 4, 4, generator=g).cuda()
    for xx, a, b in ((x.half(), bf_in, bf_out), (x.bfloat16(), hf_in, hf_out),          # planes of the other 16-bit type
                     (x.half(), hf_in, bf_out), (x.bfloat16(), bf_in, hf_out)):
        with pytest.raises(TadmmError):
            ops.chain_fused(xx, a, b, bias, 24)
    with pytest.raises(TadmmError):
        ops.chain_single(x.half(), bf_in, None, 32)
    with pytest.raises(TadmmError):
        ops.chain_single(x.bfloat16(), hf_in, None, 32)
    with pytest.raises(TadmmError):
        ops.svd_conv(img.half(), bf_in, bf_out, bias, 24)
    with pytest.raises(TadmmError):
        ops.svd_conv(img.bfloat16(), hf_in, hf_out, bias, 24)
    with pytest.raises(TadmmError):
        ops.weight_planes(win, 3, dtype=F16)
    with pytest.raises(TadmmError):
        ops.conv_core_planes(torch.randn(8, 8, 3, 3, device="cuda"), 3, dtype=F16)
    with pytest.raises(TadmmError):
        ops.weight_planes(win, 1, dtype=torch.float32)
    # token rows whose length is no whole number of 16-byte vectors: refused by the library, as for bf16
    w12 = torch.randn(16, 12, generator=g).cuda()
    x12 = torch.randn(10, 12, generator=g).cuda()
    for dt in (F16, torch.bfloat16):
        with pytest.raises(TadmmError):
            ops.chain_single(x12.to(dt), ops.weight_planes(w12, 1, dtype=dt), None, 16)
    # the same through the C ABI with an output of our own: nothing may be written
    y = torch.full((10, 16), 7.0, dtype=F16, device="cuda")
    wp = ops.weight_planes(w12, 1, dtype=F16)
    h = ops.Handle.get(torch.cuda.current_device())
    d = _cabi.ChainDesc()
    xh = x12.half().contiguous()
    d.X, d.Y, d.Win = xh.data_ptr(), y.data_ptr(), wp.data_ptr()
    d.T, d.Kin, d.R, d.Nout = 10, 12, 16, 0
    d.ldx, d.ldy, d.win_plane = 12, 16, wp[0].numel()
    d.dtype = _cabi.CHAIN_F16
    assert h.lib.tadmm_ttconv_chain_in(h.ptr, C.byref(d), 0) == -1
    d.Kin, d.ldx, d.dtype = 16, 16, 3                                    # a dtype nobody knows
    assert h.lib.tadmm_ttconv_chain_in(h.ptr, C.byref(d), 0) == -1
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full((10, 16), 7.0, dtype=F16, device="cuda"))
    # and the operands that were refused still work where they belong
    yb = ops.chain_fused(x.bfloat16(), bf_in, bf_out, bias, 24)
    yh = ops.chain_fused(x.half(), hf_in, hf_out, bias, 24)
    assert yb.dtype == torch.bfloat16 and yh.dtype == F16
    assert (yb.float() - yh.float()).abs().max().item() < 0.1
