"""`tadmm_ttconv_fused_plan` (host only, no device) -- called raw, and through `ops._conv_chain_plan` for the forward and
`ops._conv_chain_bwd_plan` / `ops.conv_chain_bwd_fits` for the data gradient -- against the independent Python statement
of the same tile rule kept in this file, over a grid of planes, kernels, strides, ranks and both dtypes; and the three
symbols in the library."""
import ctypes as C
import itertools

import pytest
import torch

PLANES = [(7, 7), (8, 8), (14, 14), (28, 28), (56, 56), (6, 10), (2, 64), (2, 65), (64, 7), (65, 65), (9, 33)]
RANKS = [16, 20, 64, 100, 220, 256, 264]


def _conv_tile_plan(dtype, rows: int, width: int, r_halo: int, r_tile: int, halo_rows, halo_width: int,
                    extra_per_pixel: int = 0):
    """The tile search of the one-launch factorised convolution and of its data gradient: (pixels per workgroup, rows per
    workgroup, halo tiles, workgroups per image) or None.  A workgroup takes a run of whole rows of the `rows` x `width`
    plane it writes, at most tm = 64 (else 32) pixels; `halo_rows(tr)` rows of `halo_width` pixels of the plane it reads
    feed a run of tr rows, in at most three tiles of tm pixels.  The intermediate of rank `r_halo` is held for the halo, that
    of rank `r_tile` for the tile; `extra_per_pixel`: further LDS bytes per tile pixel."""
    r_halo, r_tile = -(-r_halo // 32) * 32, -(-r_tile // 32) * 32
    if r_halo > 256 or r_tile > 256:
        return None
    planes, kc = (3, 64) if dtype == torch.float32 else (1, 128)
    for tm in (64, 32):                                  # pixels per workgroup: 64, or 32 when 64 does not fit the LDS
        if width > tm:
            continue
        tr, nt = min(rows, tm // width), 0
        while tr >= 1:
            nt = -(-(halo_rows(tr) * halo_width) // tm)
            if nt <= 3:
                break
            tr -= 1
        if tr < 1:
            continue
        lds = (2 * planes * tm * (kc + 8) + planes * tm * nt * (r_halo + 8) + planes * tm * (r_tile + 8)) * 2 \
            + extra_per_pixel * tm
        if lds <= 160 * 1024:
            return tm, tr, nt, -(-rows // tr)
    return None


def _py_plan(x_shape, dtype, r1, r2, kernel_size, stride, padding, dilation, bwd):
    """The rule of the forward (tile: output rows, halo: the input rows the taps reach) and of the data gradient (tile: dX
    rows, halo: the dY rows the taps reach; the tap table joins the LDS), stated without the library."""
    from tadmm import ops
    H, W = x_shape[2], x_shape[3]
    ho, wo = ops._conv_out_hw(H, W, kernel_size, stride, padding, dilation)
    if ho <= 0 or wo <= 0 or H <= 0 or W <= 0:
        return None
    if not bwd:
        return _conv_tile_plan(dtype, ho, wo, r1, r2,
                               lambda tr: min(H, (tr - 1) * stride[0] + (kernel_size[0] - 1) * dilation[0] + 1), W)
    return _conv_tile_plan(dtype, H, W, r2, r1,
                           lambda tr: min(ho, (tr - 1 + (kernel_size[0] - 1) * dilation[0]) // stride[0] + 1), wo,
                           extra_per_pixel=kernel_size[0] * kernel_size[1] * 2)


def _c_plan(lib, x_shape, dtype, r1, r2, k, s, p, dl, mode):
    from tadmm import _cabi, ops
    d = _cabi.ConvChainDesc()
    d.dtype = _cabi.CHAIN_F32 if dtype == torch.float32 else _cabi.CHAIN_BF16
    d.B, d.C, d.H, d.W = x_shape
    d.Nout = 24
    d.R1, d.R2 = -(-r1 // 32) * 32, -(-r2 // 32) * 32
    d.Ho, d.Wo = ops._conv_out_hw(d.H, d.W, k, s, p, dl)
    d.kh, d.kw, d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = k + s + p + dl
    out = [C.c_int() for _ in range(4)]
    lds = C.c_size_t()
    rc = lib.tadmm_ttconv_fused_plan(C.byref(d), mode, *[C.byref(v) for v in out], C.byref(lds))
    if rc == -5:
        return None
    assert rc == 0, (rc, x_shape, k, s, p)
    assert 0 < lds.value <= 160 * 1024
    return tuple(v.value for v in out)


def _grid():
    for (h, w), k, s, r, dtype in itertools.product(PLANES, (1, 3, 5, 7), (1, 2), RANKS, (torch.float32, torch.bfloat16)):
        geom = ((k, k), (s, s), (k // 2, k // 2), (1, 1))
        ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
        if ho > 0 and wo > 0:
            yield (2, 24, h, w), dtype, r, RANKS[(RANKS.index(r) + 2) % len(RANKS)], geom
    # dilation, asymmetric taps, no padding
    for dtype in (torch.float32, torch.bfloat16):
        yield (2, 24, 9, 9), dtype, 20, 28, ((5, 5), (1, 1), (2, 2), (2, 2))
        yield (2, 24, 6, 10), dtype, 20, 28, ((1, 3), (1, 1), (0, 1), (1, 1))
        yield (2, 24, 8, 8), dtype, 20, 28, ((3, 3), (2, 2), (0, 0), (1, 1))


def test_forward_plan_agrees_with_the_python_rule():
    from tadmm import _cabi, ops
    lib = _cabi.load()
    seen = {True: 0, False: 0}
    for x_shape, dtype, r1, r2, geom in _grid():
        want = _py_plan(x_shape, dtype, r1, r2, *geom, bwd=False)
        got = _c_plan(lib, x_shape, dtype, r1, r2, *geom, _cabi.CONV_CHAIN_FWD)
        assert got == want, (x_shape, dtype, r1, r2, geom, got, want)
        via_ops = ops._conv_chain_plan(torch.empty(x_shape, dtype=dtype, device="meta"), r1, r2, *geom)
        assert via_ops == want, (x_shape, dtype, r1, r2, geom, via_ops, want)
        seen[want is not None] += 1
    assert seen[True] > 100 and seen[False] > 100


def test_backward_plan_agrees_with_the_python_rule():
    from tadmm import _cabi, ops
    lib = _cabi.load()
    seen = {True: 0, False: 0}
    for x_shape, dtype, r1, r2, geom in _grid():
        want = _py_plan(x_shape, dtype, r1, r2, *geom, bwd=True)
        got = _c_plan(lib, x_shape, dtype, r1, r2, *geom, _cabi.CONV_CHAIN_BWD)
        assert got == want, (x_shape, dtype, r1, r2, geom, got, want)
        via_ops = ops._conv_chain_bwd_plan(x_shape, dtype, r1, r2, *geom)
        assert via_ops == want, (x_shape, dtype, r1, r2, geom, via_ops, want)
        assert ops.conv_chain_bwd_fits(torch.empty(x_shape, dtype=dtype, device="meta"), r1, r2, *geom) == (got is not None)
        seen[want is not None] += 1
    assert seen[True] > 100 and seen[False] > 100


def test_plan_examples_and_bad_arguments():
    from tadmm import _cabi
    lib = _cabi.load()
    g3 = ((3, 3), (2, 2), (1, 1), (1, 1))
    # 14 x 14 -> 7 x 7: dX tiles of 4 + 4 + 4 + 2 rows, each with a one-tile halo
    assert _c_plan(lib, (2, 24, 14, 14), torch.float32, 20, 28, *g3, _cabi.CONV_CHAIN_BWD) == (64, 4, 1, 4)
    # W = 65, Wo = 33: the forward fits, the data gradient does not
    assert _c_plan(lib, (2, 8, 2, 65), torch.float32, 12, 20, *g3, _cabi.CONV_CHAIN_FWD) is not None
    assert _c_plan(lib, (2, 8, 2, 65), torch.float32, 12, 20, *g3, _cabi.CONV_CHAIN_BWD) is None
    d = _cabi.ConvChainDesc()
    assert lib.tadmm_ttconv_fused_plan(None, 0, None, None, None, None, None) == -1
    assert lib.tadmm_ttconv_fused_plan(C.byref(d), 0, None, None, None, None, None) == -1          # all-zero extents
    d.B, d.C, d.Nout, d.R1, d.R2, d.H, d.W, d.Ho, d.Wo = 1, 8, 8, 32, 32, 7, 7, 7, 7
    d.kh = d.kw = 3
    d.stride_h = d.stride_w = d.pad_h = d.pad_w = d.dil_h = d.dil_w = 1
    assert lib.tadmm_ttconv_fused_plan(C.byref(d), 2, None, None, None, None, None) == -1          # unknown mode
    assert lib.tadmm_ttconv_fused_plan(C.byref(d), 1, None, None, None, None, None) == 0           # every output is optional
    d.Ho = 8
    assert lib.tadmm_ttconv_fused_plan(C.byref(d), 0, None, None, None, None, None) == -1          # not the geometry's output


@pytest.mark.parametrize("x_shape", [(1, 8, 2 ** 31, 4), (1, 8, 4, 2 ** 31)])
def test_an_extent_beyond_int32_is_no_plan_and_no_library_call(x_shape, monkeypatch):
    """ctypes would wrap 2**31 into the descriptor's int32 fields: both plans answer None before the library is asked."""
    from tadmm import _cabi, ops

    def no_call():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_cabi, "load", no_call)
    g = ((3, 3), (1, 1), (1, 1), (1, 1))
    assert ops._conv_chain_plan(torch.empty(x_shape, dtype=torch.bfloat16, device="meta"), 32, 32, *g) is None
    assert ops._conv_chain_bwd_plan(x_shape, torch.bfloat16, 32, 32, *g) is None
    assert not ops.conv_chain_bwd_fits(torch.empty(x_shape, dtype=torch.bfloat16, device="meta"), 32, 32, *g)


def test_symbols_are_exported_and_bound():
    from tadmm import _cabi, ops
    lib = _cabi.load()
    for name in ("tadmm_ttconv_fused_save", "tadmm_ttconv_fused_bwd", "tadmm_ttconv_fused_plan"):
        assert name in _cabi.ABI and getattr(lib, name) is not None
    for fn in ("conv_chain_save", "conv_chain_bwd", "conv_chain_bwd_fits", "conv_chain_train_pays"):
        assert callable(getattr(ops, fn))


def test_routing_rule_classes():
    """`ops.conv_chain_train_pays`: host-only shape logic."""
    from tadmm import ops
    g = ((3, 3), (1, 1), (1, 1), (1, 1))

    def x(b, side, dtype):
        return torch.empty(b, 64, side, side, dtype=dtype, device="meta")
    f32, bf16 = torch.float32, torch.bfloat16
    assert ops.conv_chain_train_pays(x(32, 56, bf16), 45, 45, *g, training=False)            # frozen, bf16: always
    assert ops.conv_chain_train_pays(x(32, 28, f32), 72, 72, *g, training=False)             # 32 x 28 = 896 workgroups
    assert not ops.conv_chain_train_pays(x(32, 56, f32), 45, 45, *g, training=False)         # 32 x 56 = 1792
    assert not ops.conv_chain_train_pays(x(32, 14, f32), 64, 64, *g, training=True)          # training, fp32: never
    assert ops.conv_chain_train_pays(x(32, 32, bf16), 16, 16, *g, training=True)             # 1024 pixels
    assert not ops.conv_chain_train_pays(x(32, 56, bf16), 45, 45, *g, training=True)
    assert not ops.conv_chain_train_pays(x(32, 112, bf16), 45, 45, *g, training=False)       # the forward does not fit
