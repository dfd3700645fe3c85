"""float16 as the third activation dtype of the chain kernels, host side (no device): the ABI constant, the plan of the
one-launch convolution (TADMM_CHAIN_F16 must plan exactly as TADMM_CHAIN_BF16), and the routing rules of `tadmm.ops`,
which treat float16 as bfloat16 everywhere except the k x k core convolution."""
import ctypes as C
import itertools

import torch

PLANES = [(7, 7), (8, 8), (14, 14), (28, 28), (56, 56), (6, 10), (2, 64), (2, 65), (64, 7), (65, 65), (9, 33)]
RANKS = [16, 20, 64, 100, 220, 256, 264]


def _grid():
    for (h, w), k, s, r in itertools.product(PLANES, (1, 3, 5, 7), (1, 2), RANKS):
        geom = ((k, k), (s, s), (k // 2, k // 2), (1, 1))
        ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
        if ho > 0 and wo > 0:
            yield (2, 24, h, w), r, RANKS[(RANKS.index(r) + 2) % len(RANKS)], geom
    yield (2, 24, 9, 9), 20, 28, ((5, 5), (1, 1), (2, 2), (2, 2))           # dilation
    yield (2, 24, 6, 10), 20, 28, ((1, 3), (1, 1), (0, 1), (1, 1))          # asymmetric taps
    yield (2, 24, 8, 8), 20, 28, ((3, 3), (2, 2), (0, 0), (1, 1))           # no padding


def _c_plan(lib, cdtype, x_shape, r1, r2, k, s, p, dl, mode):
    """(status, tile pixels, tile rows, halo tiles, tiles per image, LDS bytes) of `tadmm_ttconv_fused_plan`."""
    from tadmm import _cabi, ops
    d = _cabi.ConvChainDesc()
    d.dtype = cdtype
    d.B, d.C, d.H, d.W = x_shape
    d.Nout = 24
    d.R1, d.R2 = -(-r1 // 32) * 32, -(-r2 // 32) * 32
    d.Ho, d.Wo = ops._conv_out_hw(d.H, d.W, k, s, p, dl)
    d.kh, d.kw, d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.dil_h, d.dil_w = k + s + p + dl
    out = [C.c_int(-7) for _ in range(4)]
    lds = C.c_size_t(0)
    rc = lib.tadmm_ttconv_fused_plan(C.byref(d), mode, *[C.byref(v) for v in out], C.byref(lds))
    return (rc,) + tuple(v.value for v in out) + (lds.value,)


def test_abi_constant():
    from tadmm import _cabi
    assert _cabi.CHAIN_F16 == 2
    assert (_cabi.CHAIN_F32, _cabi.CHAIN_BF16) == (0, 1)


def test_f16_plan_equals_bf16_plan_field_for_field():
    from tadmm import _cabi
    lib = _cabi.load()
    for mode in (_cabi.CONV_CHAIN_FWD, _cabi.CONV_CHAIN_BWD):
        seen = {True: 0, False: 0}
        for x_shape, r1, r2, geom in _grid():
            bf = _c_plan(lib, _cabi.CHAIN_BF16, x_shape, r1, r2, *geom, mode)
            hf = _c_plan(lib, _cabi.CHAIN_F16, x_shape, r1, r2, *geom, mode)
            assert bf[0] in (0, -5), (bf, x_shape, geom)
            assert hf == bf, (x_shape, r1, r2, geom, mode, hf, bf)
            seen[bf[0] == 0] += 1
        assert seen[True] > 50 and seen[False] > 50
    # an unknown dtype is still refused
    assert _c_plan(lib, 3, (2, 24, 7, 7), 20, 28, (3, 3), (1, 1), (1, 1), (1, 1), _cabi.CONV_CHAIN_FWD)[0] == -1


def test_python_plan_for_float16_is_the_bfloat16_plan():
    from tadmm import ops
    for x_shape, r1, r2, geom in _grid():
        hf = ops._conv_chain_plan(torch.empty(x_shape, dtype=torch.float16, device="meta"), r1, r2, *geom)
        bf = ops._conv_chain_plan(torch.empty(x_shape, dtype=torch.bfloat16, device="meta"), r1, r2, *geom)
        assert hf == bf, (x_shape, r1, r2, geom)


def test_routing_rules_treat_float16_as_bfloat16():
    from tadmm import ops
    g1 = ((3, 3), (1, 1), (1, 1), (1, 1))
    x = torch.zeros(2, 64, 8, 8)
    big = torch.zeros(2, 64, 28, 28)
    cases = [(x, 23, 25, g1), (x, 220, 220, g1), (torch.zeros(2, 64, 14, 14), 250, 250, ((5, 5), (1, 1), (2, 2), (1, 1))),
             (torch.zeros(2, 64, 14, 14), 23, 25, g1), (torch.zeros(2, 8, 112, 112), 8, 8, g1),
             (torch.zeros(2, 8, 56, 56), 8, 8, ((7, 7), (1, 1), (3, 3), (1, 1))), (x, 300, 25, g1),
             (x, 23, 25, ((3, 3), (2, 2), (1, 1), (1, 1))), (x, 23, 25, ((9, 9), (1, 1), (0, 0), (1, 1))), (big, 72, 72, g1)]
    fits = []
    for t, r1, r2, g in cases:
        assert ops.conv_chain_fits(t.half(), r1, r2, *g) == ops.conv_chain_fits(t.bfloat16(), r1, r2, *g)
        assert ops.conv_chain_pays(t.half(), r1, r2, *g) == ops.conv_chain_pays(t.bfloat16(), r1, r2, *g)
        fits.append(ops.conv_chain_fits(t.half(), r1, r2, *g))
    assert any(fits) and not all(fits)
    assert ops.conv_chain_pays(big.half(), 72, 72, *g1) and not ops.conv_chain_pays(big, 72, 72, *g1)
    for rank in (0, 1, 20, 256, 257):
        assert ops.svd_conv_pays(x.half(), rank) == ops.svd_conv_pays(x.bfloat16(), rank)
    assert ops.svd_conv_pays(x.half(), 20) and not ops.svd_conv_pays(x, 20)


def test_float16_stays_off_the_core_convolution_and_the_training_route():
    from tadmm import ops
    g1 = ((3, 3), (1, 1), (1, 1), (1, 1))
    x = torch.zeros(2, 64, 8, 8)
    assert ops.core_conv_fits(x.bfloat16(), 25, *g1)
    assert not ops.core_conv_fits(x.half(), 25, *g1)
    assert not ops.core_conv_pays(x.half(), 25, *g1)
    for training in (False, True):                       # no saved intermediates and no data gradient in float16
        assert not ops.conv_chain_train_pays(x.half(), 23, 25, *g1, training=training)
    assert not ops.conv_chain_bwd_fits(x.half(), 23, 25, *g1)
