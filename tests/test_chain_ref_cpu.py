"""The yardsticks of tests/test_gpu_chain_variants.py must discriminate before they judge a kernel: CPU models of the
chain kernels' arithmetic (tests/_chain_ref.py) pass the criteria as built and fail them with one deliberate fault each.
No GPU, no library.

Figures of these cases (printed with -s): the full three-plane emulation has an rms error of 0.39 - 0.44 of a float32
matmul's and uses at most 0.004 of the elementwise bound; without one of the 2^-16 pairs the rms ratio is 9 - 21 (their
elementwise error stays at 0.003 - 0.13 of the bound: only the rms criterion sees them); without one of the 2^-8 pairs
the elementwise error is 2.1 - 80 times the bound."""
import pytest
import torch

from _chain_ref import (KEPT_PAIRS, guarded, guards_intact, half_chain_model, linear_bound, linear_bound_f32,
                        rms_ratio_vs_fp32, same_bits, split3, three_plane_chain, three_plane_emulation, untouched, SENTINEL)

SHAPES = [(133, 200, 81, 403), (69, 72, 17, 408), (133, 200, 256, 403)]
_CASES = {}


def _case(shape):
    """randn inputs, factors scaled by 1 / sqrt(K); built once per shape and never modified."""
    if shape not in _CASES:
        T, kin, r, nout = shape
        g = torch.Generator().manual_seed(T + kin + r)
        x = torch.randn(T, kin, generator=g)
        win = torch.randn(r, kin, generator=g) / kin ** 0.5
        wout = torch.randn(nout, r, generator=g) / r ** 0.5
        bias = torch.randn(nout, generator=g)
        _CASES[shape] = (x, [win, wout], bias, linear_bound_f32(x, [win, wout], bias))
    return _CASES[shape]


def _worst(y, ref, bound):
    return ((y.double() - ref).abs() / bound).max().item()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_full_three_plane_emulation_passes_both_criteria(shape):
    x, ws, bias, (ref, bound) = _case(shape)
    y = three_plane_chain(x, ws, bias)
    ratio, worst = rms_ratio_vs_fp32(y, x, ws, bias), _worst(y, ref, bound)
    print(f"three planes {shape}: rms ratio {ratio:.3f}, worst err / bound {worst:.2e}")
    assert ratio <= 2.0 and worst <= 1.0


@pytest.mark.parametrize("drop", KEPT_PAIRS[:3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rms_criterion_fails_without_a_low_order_pair(shape, drop):
    x, ws, bias, (ref, bound) = _case(shape)
    y = three_plane_chain(x, ws, bias, drop=drop)
    ratio = rms_ratio_vs_fp32(y, x, ws, bias)
    print(f"three planes {shape} without {drop}: rms ratio {ratio:.2f}, worst err / bound {_worst(y, ref, bound):.2e}")
    assert ratio > 2.0


@pytest.mark.parametrize("drop", ["x2y1", "x1y2"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_elementwise_bound_fails_without_a_second_order_pair(shape, drop):
    x, ws, bias, (ref, bound) = _case(shape)
    worst = _worst(three_plane_chain(x, ws, bias, drop=drop), ref, bound)
    print(f"three planes {shape} without {drop}: worst err / bound {worst:.2f}")
    assert worst > 1.0


def test_emulation_is_the_exact_split_and_a_single_product():
    x, ws, _, _ = _case(SHAPES[1])
    for a in (x, ws[0]):
        p = split3(a)
        assert all(torch.equal(t, t.bfloat16().float()) for t in p)
        assert bool((p[1].abs() <= 2.0 ** -8 * a.abs()).all()) and bool((p[2].abs() <= 2.0 ** -16 * a.abs()).all())
    y = three_plane_emulation(x, ws[0])
    ref, bound = linear_bound_f32(x, [ws[0]], None)
    assert y.shape == (x.shape[0], ws[0].shape[0]) and _worst(y, ref, bound) <= 1.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_plane_model_inside_the_bound_and_its_faults_outside(shape, dtype):
    x, ws, bias, _ = _case(shape)
    worst = {}
    for fault in (None, "mid_twice", "skip_kstep"):
        y, xq, wq = half_chain_model(x, ws, bias, dtype, fault)
        assert y.dtype == dtype
        ref, bound = linear_bound(xq, wq, bias, dtype)
        worst[fault] = _worst(y, ref, bound)
    print(f"one plane {dtype} {shape}: worst err / bound {worst}")
    assert worst[None] <= 1.0
    assert worst["mid_twice"] > 1.0
    assert worst["skip_kstep"] > 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_guarded_views_see_every_stray_write(dtype):
    assert float(torch.tensor(SENTINEL).to(dtype)) == SENTINEL
    epl = 16 // torch.empty((), dtype=dtype).element_size()
    for shape, ld, off in (((5, 12), None, 0), ((5, 12), 12 + epl, 0), ((5, 12), 13, 1), ((2, 3, 8), None, 1)):
        v = guarded(shape, dtype, ld=ld, off=off, device="cpu")
        assert tuple(v.shape) == shape and untouched(v) and guards_intact(v)
        assert v.data_ptr() % 16 == off * v.element_size()
        if len(shape) == 2:
            assert v.stride() == (ld or shape[1], 1)
        v.zero_()                                                  # writing the view itself leaves the guards alone
        assert guards_intact(v) and not untouched(v)
        base, s = v._base, v.storage_offset()
        stray = [s - 1, s + (v.numel() if v.dim() != 2 else (shape[0] - 1) * v.stride(0) + shape[1])]
        if len(shape) == 2 and v.stride(0) > shape[1]:
            stray.append(s + shape[1])                             # first element of the gap behind row 0
        for i in stray:
            base[i] = 1.0
            assert not guards_intact(v), (shape, ld, off, i)
            base[i] = SENTINEL
        assert guards_intact(v)
    a = torch.tensor([1.0, -0.0], dtype=dtype)
    assert same_bits(a, a.clone()) and not same_bits(a, torch.tensor([1.0, 0.0], dtype=dtype))
