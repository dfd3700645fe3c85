"""Every instantiation of the forward-chain kernels (csrc/chain.hip) against float64, ELEMENTWISE, at the smallest shapes
that reach the edges.  60 kernels: {f32, bf16, f16} x {32, 64}-token tiles x padded middle rank {64, 128, 192, 256} x
{token rows, NCHW images} fused chains, and 3 x 4 single products; the case ids spell dtype-tile-rank / dtype-layout.

Criteria (tests/_chain_ref.py; tests/test_chain_ref_cpu.py shows that they discriminate): the derived elementwise bound
of the dtype; for float32 also rms(error) <= 2 x rms(error of a float32 matmul) -- the elementwise bound of a sum is too
loose to see a dropped 2^-16 plane pair, the rms ratio sees it (9 - 21 in the CPU model); bitwise equality between the
entries that share a kernel; agreement of the two token tiles inside the sum of their bounds.

Shapes.  Token rows: T = 2 * tile + 5 (three workgroups, so the chunk and group rotations take 0, 1, 2; ragged last
tile), Kin = 200 (ragged last chunk for KC = 64 and 128, ragged last k-step, 200 % 8 == 0), true rank R_pad - 47 (no
multiple of 16) and 256, Nout = 408 (more than four feature groups of 48 and of 96: the second output pass; vector
epilogue) and 403 (ragged last tile, element epilogue).  Images: 3 x 72 channels, planes of 49 (scalar, straddled
tiles), 36 (vector for float32 only) and 64 pixels (vector for all), C_out = 100 (second staging pass) and 403.

Views (d) and the partial-plane descriptor (e) go through the raw C ABI with outputs cut out of sentinel-filled buffers:
every variant must give the bits of its contiguous twin and leave every guard element alone; every refusal must return
its status and write nothing."""
import functools
import gc

import pytest
import torch

from _chain_ref import (DTYPES, PLANES, bound_of, guarded, guards_intact, image_rows, launch_desc, report,
                        rms_ratio_vs_fp32, same_bits, untouched)

pytestmark = pytest.mark.gpu

KIN, NOUTS = 200, (408, 403)
IMG_B, IMG_C, PLANES_HW = 3, 72, ((7, 7), (6, 6), (8, 8))
RPADS = (64, 128, 192, 256)
ERR_INVALID = -1


def _ops():
    from tadmm import ops
    return ops


def _pdt(dtype):
    return torch.float16 if dtype == torch.float16 else torch.bfloat16


def _ranks(rpad):
    return (rpad - 47,) + ((256,) if rpad == 256 else ())


# ------------------------------------------------------------------ operands and references, built once, never modified
@functools.lru_cache(maxsize=None)
def _rows(T, kin, dtype):
    g = torch.Generator(device="cpu").manual_seed(1000 + kin)
    return torch.randn(133, kin, generator=g)[:T].cuda().to(dtype).contiguous()


@functools.lru_cache(maxsize=None)
def _image(hw, c, dtype):
    g = torch.Generator(device="cpu").manual_seed(2000 + hw[0] * hw[1] + c)
    return torch.randn(IMG_B, c, *hw, generator=g).cuda().to(dtype)


@functools.lru_cache(maxsize=None)
def _fused_weights(kin, r, nout, dtype):
    """(Win planes, Wout planes, bias, [the weights the kernel multiplies])."""
    ops = _ops()
    g = torch.Generator(device="cpu").manual_seed(kin * 7 + r * 3 + nout)
    win = (torch.randn(r, kin, generator=g) / kin ** 0.5).cuda()
    wout = (torch.randn(nout, r, generator=g) / r ** 0.5).cuda()
    bias = torch.randn(nout, generator=g).cuda()
    P = PLANES[dtype]
    wp_in = ops.weight_planes(win, P, pad_rows=64, dtype=_pdt(dtype))
    wp_out = ops.weight_planes(wout, P, pad_cols=64, dtype=_pdt(dtype))
    eff = [ops.unpack_planes(wp_in).float().sum(0)[:r, :kin], ops.unpack_planes(wp_out).float().sum(0)[:nout, :r]]
    if P == 3:
        assert torch.equal(eff[0], win) and torch.equal(eff[1], wout)        # the three planes are the weight, exactly
    return wp_in, wp_out, bias, eff


@functools.lru_cache(maxsize=None)
def _single_weights(kin, n, dtype):
    ops = _ops()
    g = torch.Generator(device="cpu").manual_seed(kin * 11 + n)
    w = (torch.randn(n, kin, generator=g) / kin ** 0.5).cuda()
    bias = torch.randn(n, generator=g).cuda()
    wp = ops.weight_planes(w, PLANES[dtype], dtype=_pdt(dtype))
    return wp, bias, [ops.unpack_planes(wp).float().sum(0)[:n, :kin]]


@functools.lru_cache(maxsize=None)
def _fused_rows_ref(r, nout, has_bias, dtype):
    _, _, bias, eff = _fused_weights(KIN, r, nout, dtype)
    return bound_of(_rows(133, KIN, dtype), eff, bias if has_bias else None, dtype)


@functools.lru_cache(maxsize=None)
def _fused_img_ref(hw, r, nout, has_bias, dtype):
    _, _, bias, eff = _fused_weights(IMG_C, r, nout, dtype)
    return bound_of(image_rows(_image(hw, IMG_C, dtype)), eff, bias if has_bias else None, dtype)


@functools.lru_cache(maxsize=None)
def _single_ref(hw, kin, n, has_bias, dtype):
    _, bias, eff = _single_weights(kin, n, dtype)
    return bound_of(image_rows(_image(hw, kin, dtype)), eff, bias if has_bias else None, dtype)


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    """The cached operands and references live as long as this module and no longer, and the blocks they used go back
    to the device: later test files measure the allocator (peak memory of a launch), and must find it as if this file
    had not run."""
    yield
    for cached in (_rows, _image, _fused_weights, _single_weights, _fused_rows_ref, _fused_img_ref, _single_ref):
        cached.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


def _judge(name, y, ref, bound, dtype, x, eff, bias):
    """Elementwise bound for every dtype (prints its figures first); float32 also the rms ratio against a plain matmul."""
    report(name, y, ref, bound)
    if dtype == torch.float32:
        ratio = rms_ratio_vs_fp32(y, x, eff, bias)
        print(f"fp32 {name}: rms ratio {ratio:.3f}")
        assert ratio <= 2.0, (name, ratio)


FUSED = [(dn, tile, rpad) for dn in DTYPES for tile in (32, 64) for rpad in RPADS]
FUSED_IDS = [f"{dn}-tile{tile}-R{rpad}" for dn, tile, rpad in FUSED]


# ------------------------------------------------------------------ a. fused chain on token rows
def _fused_rows(dn, tile, r, nout, has_bias, entry="tadmm_ttlinear_fwd"):
    dtype = DTYPES[dn]
    wp_in, wp_out, bias, _ = _fused_weights(KIN, r, nout, dtype)
    x = _rows(2 * tile + 5, KIN, dtype)
    return _ops().chain_fused(x, wp_in, wp_out, bias if has_bias else None, nout, entry=entry, tile_tokens=tile)


@pytest.mark.parametrize("dn,tile,rpad", FUSED, ids=FUSED_IDS)
def test_fused_rows(dn, tile, rpad):
    dtype, T = DTYPES[dn], 2 * tile + 5
    for r in _ranks(rpad):
        for nout in NOUTS:
            for has_bias in (True, False):
                wp_in, _, bias, eff = _fused_weights(KIN, r, nout, dtype)
                assert wp_in.shape[1] * 16 == rpad
                y = _fused_rows(dn, tile, r, nout, has_bias)
                assert y.shape == (T, nout) and y.dtype == dtype
                ref, bound = _fused_rows_ref(r, nout, has_bias, dtype)
                _judge(f"a {dn} tile {tile} R {rpad} r {r} N {nout} bias {int(has_bias)}", y, ref[:T], bound[:T], dtype,
                       _rows(T, KIN, dtype), eff, bias if has_bias else None)
                assert same_bits(_fused_rows(dn, tile, r, nout, has_bias, "tadmm_ttlinear_bwd"), y)
                # the other tile computes the same rows in another order: inside the sum of the two bounds
                To = min(T, 2 * (96 - tile) + 5)
                yo = _fused_rows(dn, 96 - tile, r, nout, has_bias)
                gap = ((y[:To].double() - yo[:To].double()).abs() / (2 * bound[:To])).max().item()
                assert gap <= 1.0, (dn, tile, r, nout, gap)


# ------------------------------------------------------------------ b. fused chain on images
def _fused_img(dn, tile, hw, r, nout, has_bias, entry="tadmm_svdconv_fwd"):
    dtype = DTYPES[dn]
    wp_in, wp_out, bias, _ = _fused_weights(IMG_C, r, nout, dtype)
    return _ops().svd_conv(_image(hw, IMG_C, dtype), wp_in, wp_out, bias if has_bias else None, nout, entry=entry,
                           tile_tokens=tile)


@pytest.mark.parametrize("dn,tile,rpad", FUSED, ids=FUSED_IDS)
def test_fused_images(dn, tile, rpad):
    dtype = DTYPES[dn]
    for r in _ranks(rpad):
        for hw in PLANES_HW:
            for nout, has_bias in ((100, True), (100, False)) + (((403, True),) if rpad == 128 else ()):
                _, _, bias, eff = _fused_weights(IMG_C, r, nout, dtype)
                y = _fused_img(dn, tile, hw, r, nout, has_bias)
                assert y.shape == (IMG_B, nout, *hw) and y.dtype == dtype
                ref, bound = _fused_img_ref(hw, r, nout, has_bias, dtype)
                _judge(f"b {dn} tile {tile} R {rpad} r {r} hw {hw[0] * hw[1]} N {nout} bias {int(has_bias)}", image_rows(y),
                       ref, bound, dtype, image_rows(_image(hw, IMG_C, dtype)), eff, bias if has_bias else None)
                assert same_bits(_fused_img(dn, tile, hw, r, nout, has_bias, "tadmm_svdconv_bwd"), y)
                yo = _fused_img(dn, 96 - tile, hw, r, nout, has_bias)
                gap = ((image_rows(y).double() - image_rows(yo).double()).abs() / (2 * bound)).max().item()
                assert gap <= 1.0, (dn, tile, r, hw, nout, gap)


# ------------------------------------------------------------------ c. single product, four layouts
SINGLE = [(dn, layout) for dn in DTYPES for layout in ("rows-rows", "image-rows", "image-image", "rows-image")]
ENTRIES = ("tadmm_ttconv_chain_in", "tadmm_ttconv_chain_out", "tadmm_tucker_1x1")


def _single(dn, layout, entry, hw, kin, n, has_bias):
    """One single-product launch; the result as token rows (B*hw, n) whatever the layout."""
    ops, dtype = _ops(), DTYPES[dn]
    wp, bias, _ = _single_weights(kin, n, dtype)
    b = bias if has_bias else None
    ximg = _image(hw, kin, dtype)
    src, dst = layout.split("-")
    x = ximg if src == "image" else image_rows(ximg).contiguous()
    if layout == "rows-image":                                      # `ops` cannot express it: the raw descriptor
        y = torch.empty(IMG_B, n, *hw, dtype=dtype, device="cuda")
        assert launch_desc(entry, x, y, wp, None, b, x.shape[0], kin, n, 0, ldx=kin, y_hw=hw[0] * hw[1]) == 0
    else:
        y = ops.chain_single(x, wp, b, n, entry=entry, image_out=(dst == "image"))
    assert y.dtype == dtype and y.shape == ((IMG_B, n, *hw) if dst == "image" else (IMG_B * hw[0] * hw[1], n))
    return image_rows(y) if dst == "image" else y


@pytest.mark.parametrize("dn,layout", SINGLE, ids=[f"{dn}-{layout}" for dn, layout in SINGLE])
def test_single_product(dn, layout):
    dtype = DTYPES[dn]
    for kin in (72, 200):
        has_bias = kin == 200
        for n in (300, 37):                                         # 300: two feature blocks (blockIdx.y = 1)
            _, bias, eff = _single_weights(kin, n, dtype)
            for hw in PLANES_HW:
                ref, bound = _single_ref(hw, kin, n, has_bias, dtype)
                y = _single(dn, layout, ENTRIES[0], hw, kin, n, has_bias)
                _judge(f"c {dn} {layout} K {kin} n {n} hw {hw[0] * hw[1]}", y, ref, bound, dtype,
                       image_rows(_image(hw, kin, dtype)), eff, bias if has_bias else None)
                for entry in ENTRIES[1:]:
                    assert same_bits(_single(dn, layout, entry, hw, kin, n, has_bias), y), entry
                if layout != "rows-rows":                            # the four layouts are one product
                    assert same_bits(_single(dn, "rows-rows", ENTRIES[0], hw, kin, n, has_bias).contiguous(),
                                     y.contiguous())


# ------------------------------------------------------------------ d. views, guards, refusals
@pytest.mark.parametrize("dn", list(DTYPES))
def test_row_views_give_the_bits_of_the_contiguous_twin(dn):
    ops, dtype = _ops(), DTYPES[dn]
    epl = 16 // torch.empty((), dtype=dtype).element_size()
    T, r, N = 69, 17, 408
    wp_in, wp_out, bias, _ = _fused_weights(KIN, r, N, dtype)
    x = _rows(T, KIN, dtype)
    twin = ops.chain_fused(x, wp_in, wp_out, bias, N)
    # X: an aligned strided row view goes through `ops` as it is, no copy
    xv = guarded((T, KIN), dtype, ld=KIN + 8)
    xv.copy_(x)
    assert xv.storage_offset() > 0 and xv.data_ptr() % 16 == 0 and not xv.is_contiguous()
    y = ops.chain_fused(xv, wp_in, wp_out, bias, N)
    key, memo = next(reversed(ops._CHAIN_MEMO.items()))
    assert key[2] == KIN + 8 and memo[0].ldx == KIN + 8 and memo[0].X == xv.data_ptr()
    assert same_bits(y, twin) and guards_intact(xv)
    # Y: padded rows (vector epilogue), the same one element off alignment (direct stores), an odd row stride
    for ld, off in ((N + epl, 0), (N + epl, 1), (N + 1, 0)):
        yv = guarded((T, N), dtype, ld=ld, off=off)
        assert launch_desc("tadmm_ttlinear_fwd", xv, yv, wp_in, wp_out, bias, T, KIN, 64, N, ldx=KIN + 8, ldy=ld) == 0
        torch.cuda.synchronize()
        assert same_bits(yv, twin), (ld, off)
        assert guards_intact(yv), (ld, off)
    # single product, rows to rows, through the same views
    wp, b1, _ = _single_weights(KIN, 300, dtype)
    twin1 = ops.chain_single(x, wp, b1, 300)
    for ld, off in ((300 + epl, 0), (300 + epl, 1), (301, 0)):
        yv = guarded((T, 300), dtype, ld=ld, off=off)
        assert launch_desc("tadmm_tucker_1x1", xv, yv, wp, None, b1, T, KIN, 300, 0, ldx=KIN + 8, ldy=ld) == 0
        torch.cuda.synchronize()
        assert same_bits(yv, twin1) and guards_intact(yv), (ld, off)


@pytest.mark.parametrize("dn", list(DTYPES))
def test_image_outputs_give_the_bits_of_the_aligned_twin(dn):
    ops, dtype = _ops(), DTYPES[dn]
    hw, r, N = (8, 8), 17, 100
    wp_in, wp_out, bias, _ = _fused_weights(IMG_C, r, N, dtype)
    x = _image(hw, IMG_C, dtype)
    twin = ops.svd_conv(x, wp_in, wp_out, bias, N)
    wp, b1, _ = _single_weights(IMG_C, 37, dtype)
    twin1 = ops.chain_single(x, wp, b1, 37, image_out=True)
    xrows = image_rows(x).contiguous()
    for off in (0, 1):                                              # 1: no 16-byte units, every pixel on its own
        yv = guarded((IMG_B, N, *hw), dtype, off=off)
        assert launch_desc("tadmm_svdconv_fwd", x, yv, wp_in, wp_out, bias, IMG_B * 64, IMG_C, 64, N, x_hw=64, y_hw=64) == 0
        torch.cuda.synchronize()
        assert same_bits(yv, twin) and guards_intact(yv), off
        for xx, x_hw, ldx in ((x, 64, 0), (xrows, 0, IMG_C)):       # image -> image and rows -> image
            yv = guarded((IMG_B, 37, *hw), dtype, off=off)
            assert launch_desc("tadmm_ttconv_chain_out", xx, yv, wp, None, b1, IMG_B * 64, IMG_C, 37, 0, ldx=ldx, x_hw=x_hw,
                               y_hw=64) == 0
            torch.cuda.synchronize()
            assert same_bits(yv, twin1) and guards_intact(yv), (off, x_hw)


@pytest.mark.parametrize("dn", list(DTYPES))
def test_refused_descriptors_write_nothing(dn):
    dtype = DTYPES[dn]
    epl = 16 // torch.empty((), dtype=dtype).element_size()
    T, r, N = 69, 17, 408
    wp_in, wp_out, bias, _ = _fused_weights(KIN, r, N, dtype)
    x = _rows(T, KIN, dtype)
    x_off = guarded((T, KIN), dtype, ld=KIN + epl, off=1)
    x_off.copy_(x)
    bias_off = torch.zeros(N + 4, device="cuda")[1:N + 1]
    assert x_off.data_ptr() % 16 != 0 and bias_off.data_ptr() % 16 == 4
    run = functools.partial(launch_desc, "tadmm_ttlinear_fwd")
    y0 = guarded((T, N), dtype, ld=N + epl)
    assert run(x, y0, wp_in, wp_out, bias, T, KIN, 64, N, ldx=KIN, ldy=N + epl) == 0      # the descriptor is sound
    torch.cuda.synchronize()
    assert not untouched(y0) and guards_intact(y0)
    yv = guarded((T, N), dtype, ld=N + epl)
    assert run(x_off, yv, wp_in, wp_out, bias, T, KIN, 64, N, ldx=KIN + epl, ldy=N + epl) == ERR_INVALID   # X rows unaligned
    assert run(x, yv, wp_in, wp_out, bias, T, KIN, 64, N, ldx=KIN - epl, ldy=N + epl) == ERR_INVALID       # ldx < Kin
    assert run(x, yv, wp_in, wp_out, bias, T, KIN, 64, N, ldx=KIN, ldy=N - epl) == ERR_INVALID             # ldy < N
    assert run(x, yv, wp_in, wp_out, bias_off, T, KIN, 64, N, ldx=KIN, ldy=N + epl) == ERR_INVALID         # bias unaligned
    torch.cuda.synchronize()
    assert untouched(yv) and guards_intact(yv)


# ------------------------------------------------------------------ e. a token count that is no whole number of planes
@pytest.mark.parametrize("dn", list(DTYPES))
def test_partial_image_plane_is_refused(dn):
    """With y_hw % (16-byte unit) == 0 the vector image epilogue tests `t < T` for the first pixel of a unit only: at
    y_hw = 16, T = 50 the unit of pixels 48..51 would store two pixels past T (inside the fourth plane of the buffer
    used here, so nothing is out of bounds either way).  Such a descriptor describes no tensor; every chain entry
    refuses it (include/tadmm.h), on the input side as well."""
    dtype = DTYPES[dn]
    kin, n, hw = IMG_C, 37, 16
    wp, bias, _ = _single_weights(kin, n, dtype)
    x = _rows(50, KIN, dtype)[:, :kin].contiguous()
    ximg = _image((8, 8), kin, dtype)                               # 3 x 72 x 64: holds 50 tokens of 16-pixel planes
    for entry in ENTRIES:
        yimg = guarded((4, n, 4, 4), dtype)
        assert launch_desc(entry, x, yimg, wp, None, bias, 50, kin, n, 0, ldx=kin, y_hw=hw) == ERR_INVALID
        yrow = guarded((50, n), dtype)
        assert launch_desc(entry, ximg, yrow, wp, None, bias, 50, kin, n, 0, ldy=n, x_hw=hw) == ERR_INVALID
        torch.cuda.synchronize()
        assert untouched(yimg) and guards_intact(yimg) and untouched(yrow) and guards_intact(yrow)
    # whole planes: the same descriptor with T = 48 runs and matches the rows -> rows product
    yimg = guarded((3, n, 4, 4), dtype)
    assert launch_desc(ENTRIES[0], x, yimg, wp, None, bias, 48, kin, n, 0, ldx=kin, y_hw=hw) == 0
    torch.cuda.synchronize()
    want = _ops().chain_single(x[:48], wp, bias, n)
    assert same_bits(image_rows(yimg).contiguous(), want) and guards_intact(yimg)
