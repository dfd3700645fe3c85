"""Split-T weight-gradient kernel (csrc/wgrad.hip, `ops.wgrad`) against fp64 torch on the device: parity over both
layouts and dtypes, an exactly derivable case, determinism at the C ABI, the slice decomposition, operand copies, autograd
of the factorised layers at training size, refusals.

Parity bar: max|C - C64| <= 1e-5 * max|C64| (the bar of tests/test_gpu_chain.py for gradients); for bf16 operands C64 is
formed from the bf16 values (products are exact, only the fp32 accumulation differs).  Every parity test prints the
kernel's error beside the error of the route it replaces (`ops.mm` on channel-major fp32 copies).

bf16 at training size: the convolution layers (SVDConv2dC, TKConv2dC, TTConv2dM) hand bf16 activations to the chain
kernels and so to `ops.wgrad` as bf16.  TTLinearM / TKLinearM take the fused chain for training in fp32 only; with bf16
activations and trainable cores they run their per-core `mm` chain (fp32 products), so their bf16 tests below exercise
that route, and the bf16 token-row route of `_FusedChain.backward` is tested through `functional.linear_chain` itself."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.bfloat16]


class HP:
    def __init__(self, ranks, tt_shapes=None):
        self.ranks = ranks
        self.tt_shapes = tt_shapes


def _ops():
    from tadmm import ops
    return ops


def _rel(y, ref):
    return (y.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _ref64(a, b):
    if a.dim() == 4:
        return torch.einsum("bmp,bnp->mn", a.double().flatten(2), b.double().flatten(2))
    return a.double().t() @ b.double()


def _parent(a, b):
    """What the layers did before: fp32 channel-major copies (images) and the one-workgroup-per-tile GEMM."""
    ops = _ops()
    if a.shape[0] == 0 or a.numel() == 0:
        return torch.zeros(a.shape[1], b.shape[1], device=a.device)
    if a.dim() == 4:
        a2 = a.permute(1, 0, 2, 3).reshape(a.shape[1], -1).float().contiguous()
        b2 = b.permute(1, 0, 2, 3).reshape(b.shape[1], -1).float().contiguous()
        return ops.mm(a2, b2.t())
    return ops.mm(a.float().t(), b.float())


def _check(a, b, what):
    ops = _ops()
    c = ops.wgrad(a, b)
    ref = _ref64(a, b)
    assert c.shape == ref.shape and c.dtype == torch.float32
    assert torch.isfinite(c).all()
    scale = ref.abs().max().item()
    err = (c.double() - ref).abs().max().item()
    perr = (_parent(a, b).double() - ref).abs().max().item()
    _, slices = ops.wgrad_plan(a, b)
    print(f"wgrad-parity {what} dtype={str(a.dtype)[6:]} slices={slices} err={err / max(scale, 1e-30):.3e} "
          f"parent={perr / max(scale, 1e-30):.3e}")
    assert err <= 1e-5 * scale, (what, err, scale)


# (T, M, N, lda - M, ldb - N)
ROW_CASES = [
    (0, 1, 1, 0, 0),
    (1, 10, 17, 0, 0),
    (31, 18, 24, 0, 0),
    (31, 65, 300, 3, 5),
    (12608, 64, 65, 0, 0),
    (12608, 256, 300, 0, 0),
    (12608, 24, 2048, 0, 0),
    (12608, 10, 384, 0, 0),            # the 10-class heads: rows of 10 elements, no 16-byte alignment
    (12608, 17, 18, 1, 2),             # odd strides: element loads
    (12608, 256, 384, 128, 0),         # a column block of a wider tensor
    (131072, 1, 10, 0, 0),
    (131072, 18, 24, 6, 8),
    (200704, 17, 64, 0, 0),
    (200704, 1, 1, 0, 0),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,M,N,pa,pb", ROW_CASES)
def test_rows_match_fp64(T, M, N, pa, pb, dtype):
    g = torch.Generator().manual_seed(T + 7 * M + N)
    a = torch.randn(T, M + pa, generator=g).to(DEV).to(dtype)[:, :M]
    b = torch.randn(T, N + pb, generator=g).to(DEV).to(dtype)[:, pb:]
    _check(a, b, f"rows T={T} M={M} N={N} lda={M + pa} ldb={N + pb}")


# (B, M, N, (H, W))
IMAGE_CASES = [
    (1, 18, 24, (1, 1)),
    (128, 24, 17, (1, 1)),
    (2, 65, 10, (7, 7)),
    (128, 64, 18, (7, 7)),             # 49-pixel planes: element loads, tiles cross image boundaries
    (64, 17, 24, (14, 14)),            # 196 pixels: 16-byte loads in fp32, 8-byte loads in bf16
    (3, 10, 300, (14, 14)),
    (1, 256, 65, (16, 16)),
    (128, 18, 24, (16, 16)),           # svd_mobilenetv2_cifar bottlenecks.3.conv1: dWin (T = 131 072)
    (128, 144, 18, (16, 16)),          #                                            dWout
    (2, 256, 65, (32, 32)),
    (1, 18, 24, (56, 56)),
    (8, 32, 64, (56, 56)),             # tk_resnet50 3x layer1.x.conv3: dWin
    (64, 256, 32, (56, 56)),           #                                 dWout at batch 64 (T = 200 704)
    (128, 96, 2048, (7, 7)),           # tk_resnet50 3x layer4.x.conv1: dWin
    (0, 18, 24, (16, 16)),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,M,N,hw", IMAGE_CASES)
def test_images_match_fp64(B, M, N, hw, dtype):
    g = torch.Generator().manual_seed(B + 7 * M + N + hw[0])
    a = torch.randn(B, M, *hw, generator=g).to(DEV).to(dtype)
    b = torch.randn(B, N, *hw, generator=g).to(DEV).to(dtype)
    _check(a, b, f"image B={B} M={M} N={N} hw={hw[0] * hw[1]}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,shape", [(131072, None), (200704, None), (131072, (128, 32, 32)), (200704, (64, 56, 56))])
def test_constant_operands_are_exact(T, shape, dtype):
    # 0.5 and 3.0 are exact in bf16 (so exact through the three-plane split); every partial sum is a multiple of 0.5
    # below 2^24 * 0.5, so any summation order gives 1.5 * T exactly
    M, N = 18, 24
    if shape is None:
        a = torch.full((T, M), 0.5, device=DEV, dtype=dtype)
        b = torch.full((T, N), 3.0, device=DEV, dtype=dtype)
    else:
        a = torch.full((shape[0], M, shape[1], shape[2]), 0.5, device=DEV, dtype=dtype)
        b = torch.full((shape[0], N, shape[1], shape[2]), 3.0, device=DEV, dtype=dtype)
    c = _ops().wgrad(a, b)
    assert torch.equal(c, torch.full((M, N), 1.5 * T, device=DEV))


def _abi_call(a, b, M, N, T, hw, ws_fill, c_fill, short=0):
    from tadmm import _cabi
    ops = _ops()
    h = _cabi.Handle.get(0)
    d = ops._wgrad_desc(a, b, T, M, N, hw)
    nbytes, slices = C.c_size_t(), C.c_int()
    assert h.lib.tadmm_wgrad_workspace_bytes(C.byref(d), C.byref(nbytes), C.byref(slices)) == 0
    ws = torch.full((max(nbytes.value // 4, 1),), ws_fill, device=DEV)
    out = torch.full((M, N), c_fill, device=DEV)
    d.C, d.ldc = out.data_ptr(), N
    rc = h.lib.tadmm_wgrad(h.ptr, C.byref(d), ws.data_ptr(), nbytes.value - short,
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out, nbytes.value, slices.value


@pytest.mark.parametrize("dtype", DTYPES)
def test_deterministic_and_independent_of_prior_contents(dtype):
    g = torch.Generator().manual_seed(5)
    a = torch.randn(128, 18, 32, 32, generator=g).to(DEV).to(dtype)
    b = torch.randn(128, 24, 32, 32, generator=g).to(DEV).to(dtype)
    nan = float("nan")
    rc1, c1, nbytes, slices = _abi_call(a, b, 18, 24, 131072, 1024, nan, nan)
    rc2, c2, _, _ = _abi_call(a, b, 18, 24, 131072, 1024, nan, nan)
    rc3, c3, _, _ = _abi_call(a, b, 18, 24, 131072, 1024, 0.0, 7.0)
    assert rc1 == rc2 == rc3 == 0 and slices > 1 and nbytes > 0
    assert torch.isfinite(c1).all()
    assert torch.equal(c1, c2) and torch.equal(c1, c3)
    # one slice: C written directly, the same independence
    rc4, c4, nb4, s4 = _abi_call(a[:1, :, :1, :31].contiguous(), b[:1, :, :1, :31].contiguous(), 18, 24, 31, 31, nan, nan)
    assert rc4 == 0 and s4 == 1 and nb4 == 0 and torch.isfinite(c4).all()


def test_decomposition_and_workspace_check():
    ops = _ops()
    a = torch.randn(128, 18, 32, 32, device=DEV)
    b = torch.randn(128, 24, 32, 32, device=DEV)
    nbytes, slices = ops.wgrad_plan(a, b)
    assert slices > 1 and nbytes >= slices * 18 * 24 * 4
    assert ops.wgrad_plan(a[:, :, 0, :31].reshape(-1, 18)[:31], b[:, :, 0, :31].reshape(-1, 24)[:31]) == (0, 1)
    # one byte less: TADMM_ERR_WORKSPACE and nothing launched (C keeps its fill)
    rc, out, _, _ = _abi_call(a, b, 18, 24, 131072, 1024, 0.0, 7.0, short=1)
    assert rc == -2
    assert torch.equal(out, torch.full((18, 24), 7.0, device=DEV))
    # T == 0 writes zeros
    rc, out, nb, s = _abi_call(a[:0], b[:0], 18, 24, 0, 1024, 0.0, 7.0)
    assert rc == 0 and s == 1 and nb == 0 and torch.equal(out, torch.zeros(18, 24, device=DEV))


def test_no_operand_copies():
    from tadmm import functional as HF
    ops = _ops()
    B, Cin, R, N, H, W = 64, 64, 32, 256, 56, 56           # tk_resnet50 3x layer1.x.conv3 at batch 64
    x = torch.randn(B, Cin, H, W, device=DEV)
    gr = torch.randn(B, R, H, W, device=DEV)
    ops.wgrad(gr[:1], x[:1])                                # handle, library and kernel images are loaded
    nbytes, _ = ops.wgrad_plan(gr, x)
    torch.cuda.synchronize()
    # The launch allocates from an empty pool of its own.  torch's caching allocator hands out a cached block whole when
    # what a split would leave is 1 MiB or less, and counts the whole block as allocated: a 4.7 or 5 MiB block left by
    # some earlier test, served for the 4 MiB workspace, would be measured here as if `wgrad` had asked for it.
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        c = ops.wgrad(gr, x)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
    assert rise <= 4 * R * Cin + nbytes + 2 * 512, (rise, nbytes)
    assert rise >= 4 * R * Cin + nbytes, (rise, nbytes)        # the pool's allocations are in the device-wide figures
    del c, gr, pool
    # one backward of conv1x1_chain: neither of the two channel-major copies (4 * C * B*H*W bytes each) appears
    wi = (torch.randn(R, Cin, device=DEV) / Cin ** 0.5).requires_grad_()
    wo = (torch.randn(N, R, device=DEV) / R ** 0.5).requires_grad_()
    y = HF.conv1x1_chain(x, wi, wo, None)
    gout = torch.randn_like(y)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y.backward(gout)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert rise < 4 * Cin * B * H * W, rise
    assert wi.grad is not None and wo.grad is not None


# ------------------------------------------------------------------------------------------------ autograd at size
def _grad_check(params, refs, tol):
    for (name, p), r in zip(params, refs):
        got = p.grad.double().reshape(r.grad.shape)
        err = _rel(got, r.grad)
        print(f"wgrad-autograd {name} err={err:.3e}")
        assert err < tol, (name, err)


@pytest.mark.parametrize("bf16", [False, True])
def test_svdconv2dc_mobilenetv2_batch128(bf16):
    from tadmm import svd_layers
    torch.manual_seed(11)
    layer = svd_layers.SVDConv2dC(24, 144, 1, bias=True, hp_dict=HP({"l.weight": 18}), name="l.weight").to(DEV)
    with torch.no_grad():
        layer.bias.normal_()
    x = torch.randn(128, 24, 16, 16, device=DEV)
    gout = torch.randn(128, 144, 16, 16, device=DEV)
    if bf16:
        x, gout = x.bfloat16(), gout.bfloat16()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = layer(x)
        assert y.dtype == torch.bfloat16
    else:
        y = layer(x)
    y.backward(gout)
    leaves = [t.detach().double().requires_grad_() for t in (layer.left_kernel, layer.right_kernel, layer.bias)]
    y64 = F.conv2d(F.conv2d(x.double(), leaves[0].reshape(18, 24, 1, 1)), leaves[1].reshape(144, 18, 1, 1), leaves[2])
    y64.backward(gout.double())
    _grad_check([("left_kernel", layer.left_kernel), ("right_kernel", layer.right_kernel), ("bias", layer.bias)],
                leaves, 2e-2 if bf16 else 2e-5)


@pytest.mark.parametrize("bf16", [False, True])
def test_tkconv2dc_resnet50_layer1_batch8(bf16):
    from tadmm import tk_layers
    torch.manual_seed(12)
    layer = tk_layers.TKConv2dC(64, 64, 3, padding=1, bias=True, hp_dict=HP({"l.weight": [32, 32]}), name="l.weight").to(DEV)
    with torch.no_grad():
        layer.bias.normal_()
    x = torch.randn(8, 64, 56, 56, device=DEV)
    gout = torch.randn(8, 64, 56, 56, device=DEV)
    if bf16:
        x, gout = x.bfloat16(), gout.bfloat16()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = layer(x)
    else:
        y = layer(x)
    y.backward(gout)
    names = ("first_kernel", "core_kernel", "last_kernel", "bias")
    leaves = [getattr(layer, n).detach().double().requires_grad_() for n in names]
    y64 = F.conv2d(F.conv2d(F.conv2d(x.double(), leaves[0]), leaves[1], padding=1), leaves[2], leaves[3])
    y64.backward(gout.double())
    _grad_check([(n, getattr(layer, n)) for n in names], leaves, 2e-2 if bf16 else 2e-5)


def test_ttlinearm_deit_qkv_12608_tokens():
    from tadmm import tt_layers
    torch.manual_seed(13)
    hp = HP({"qkv.weight": [1, 25, 256, 18, 1]}, {"qkv.weight": [36, 32, 16, 24]})
    lin = tt_layers.TTLinearM(384, 1152, bias=True, hp_dict=hp, name="qkv.weight").to(DEV)
    with torch.no_grad():
        lin.bias.normal_()
    x = torch.randn(64, 197, 384, device=DEV)
    y = lin(x)
    gout = torch.randn_like(y)
    y.backward(gout)
    cores = [c.detach().double().requires_grad_() for c in lin.tt_cores]
    w = cores[0].reshape(-1, cores[0].shape[-1])
    for c in cores[1:]:
        w = w.reshape(-1, c.shape[0]) @ c.reshape(c.shape[0], -1)          # ttd.py:39-40
    b64 = lin.bias.detach().double().requires_grad_()
    y64 = x.double() @ w.reshape(1152, 384).t() + b64
    y64.backward(gout.double())
    _grad_check([(f"tt_cores[{i}]", c) for i, c in enumerate(lin.tt_cores)] + [("bias", lin.bias)], cores + [b64], 2e-5)


def test_tklinearm_deit_qkv_12608_tokens():
    from tadmm import tk_layers
    torch.manual_seed(14)
    lin = tk_layers.TKLinearM(384, 1152, bias=True, hp_dict=HP({"qkv.weight": [256, 192]}), name="qkv.weight").to(DEV)
    x = torch.randn(64, 197, 384, device=DEV)
    y = lin(x)
    gout = torch.randn_like(y)
    y.backward(gout)
    names = ("first_factor", "core_tensor", "last_factor", "bias")
    leaves = [getattr(lin, n).detach().double().requires_grad_() for n in names]
    y64 = F.linear(F.linear(F.linear(x.double(), leaves[0]), leaves[1]), leaves[2], leaves[3])      # TKLinear.py:66-71
    y64.backward(gout.double())
    _grad_check([(n, getattr(lin, n)) for n in names], leaves, 2e-5)


def _recover64(cores):
    w = cores[0].reshape(-1, cores[0].shape[-1])
    for c in cores[1:]:
        w = w.reshape(-1, c.shape[0]) @ c.reshape(c.shape[0], -1)          # TTConv.py:313-319, ttd.py:39-40
    return w


@pytest.mark.parametrize("bf16", [False, True])
def test_ttconv2dm_resnet18_layer3_batch8(bf16):
    from tadmm import tt_layers
    torch.manual_seed(15)
    name = "layer3.1.conv1.weight"                                         # tt_resnet18 general 2x
    hp = HP({name: [1, 15, 138, 138, 15, 1]}, {name: [16, 16, 9, 16, 16]})
    layer = tt_layers.TTConv2dM(256, 256, 3, padding=1, bias=True, hp_dict=hp, name=name).to(DEV)
    with torch.no_grad():
        layer.bias.normal_()
    x = torch.randn(8, 256, 14, 14, device=DEV)
    gout = torch.randn(8, 256, 14, 14, device=DEV)
    if bf16:
        x, gout = x.bfloat16(), gout.bfloat16()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = layer(x)
        assert y.dtype == torch.bfloat16
    else:
        y = layer(x)
    y.backward(gout)
    ins = [c.detach().double().requires_grad_() for c in layer.in_tt_cores]
    outs = [c.detach().double().requires_grad_() for c in layer.out_tt_cores]
    core = layer.core_kernel.detach().double().requires_grad_()
    b64 = layer.bias.detach().double().requires_grad_()
    w_in = _recover64(ins).reshape(layer.in_tt_ranks[0], 256)              # TTConv.py:130-153 with the cores contracted
    w_out = _recover64(outs).reshape(256, layer.out_tt_ranks[-1])
    y64 = F.conv2d(F.conv2d(F.conv2d(x.double(), w_in[:, :, None, None]), core, padding=1), w_out[:, :, None, None], b64)
    y64.backward(gout.double())
    params = ([(f"in_tt_cores[{i}]", c) for i, c in enumerate(layer.in_tt_cores)]
              + [(f"out_tt_cores[{i}]", c) for i, c in enumerate(layer.out_tt_cores)]
              + [("core_kernel", layer.core_kernel), ("bias", layer.bias)])
    _grad_check(params, ins + outs + [core, b64], 2e-2 if bf16 else 2e-5)


def test_ttlinearm_deit_qkv_bf16_activations():
    from tadmm import tt_layers
    torch.manual_seed(16)
    hp = HP({"qkv.weight": [1, 25, 256, 18, 1]}, {"qkv.weight": [36, 32, 16, 24]})
    lin = tt_layers.TTLinearM(384, 1152, bias=True, hp_dict=hp, name="qkv.weight").to(DEV)
    with torch.no_grad():
        lin.bias.normal_()
    x = torch.randn(64, 197, 384, device=DEV).bfloat16()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = lin(x)
    gout = torch.randn(y.shape, device=DEV).to(y.dtype)
    y.backward(gout)
    cores = [c.detach().double().requires_grad_() for c in lin.tt_cores]
    b64 = lin.bias.detach().double().requires_grad_()
    y64 = x.double() @ _recover64(cores).reshape(1152, 384).t() + b64
    y64.backward(gout.double())
    _grad_check([(f"tt_cores[{i}]", c) for i, c in enumerate(lin.tt_cores)] + [("bias", lin.bias)], cores + [b64], 2e-2)


def test_tklinearm_deit_qkv_bf16_activations():
    from tadmm import tk_layers
    torch.manual_seed(17)
    lin = tk_layers.TKLinearM(384, 1152, bias=True, hp_dict=HP({"qkv.weight": [256, 192]}), name="qkv.weight").to(DEV)
    x = torch.randn(64, 197, 384, device=DEV).bfloat16()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = lin(x)
    gout = torch.randn(y.shape, device=DEV).to(y.dtype)
    y.backward(gout)
    names = ("first_factor", "core_tensor", "last_factor", "bias")
    leaves = [getattr(lin, n).detach().double().requires_grad_() for n in names]
    y64 = F.linear(F.linear(F.linear(x.double(), leaves[0]), leaves[1]), leaves[2], leaves[3])
    y64.backward(gout.double())
    _grad_check([(n, getattr(lin, n)) for n in names], leaves, 2e-2)


def test_linear_chain_bf16_token_rows_12608():
    """`_FusedChain.backward` with bf16 token rows: bf16 `gr` / `h` against bf16 `x` / `g` in `ops.wgrad` (DeiT-S qkv
    factors: Win 256 x 384, Wout 1152 x 256)."""
    from tadmm import functional as HF
    g = torch.Generator().manual_seed(18)
    x = torch.randn(12608, 384, generator=g).to(DEV).bfloat16()
    wi = (torch.randn(256, 384, generator=g) / 384 ** 0.5).to(DEV).requires_grad_()
    wo = (torch.randn(1152, 256, generator=g) / 256 ** 0.5).to(DEV).requires_grad_()
    b = torch.randn(1152, generator=g).to(DEV).requires_grad_()
    gout = torch.randn(12608, 1152, generator=g).to(DEV).bfloat16()
    y = HF.linear_chain(x, wi, wo, b)
    assert y.dtype == torch.bfloat16
    y.backward(gout)
    leaves = [t.detach().double().requires_grad_() for t in (wi, wo, b)]
    y64 = F.linear(F.linear(x.double(), leaves[0]), leaves[1], leaves[2])
    y64.backward(gout.double())
    _grad_check([("w_in", wi), ("w_out", wo), ("bias", b)], leaves, 2e-2)


def test_mm_backward_switch_is_a_function_of_the_shapes():
    from tadmm import functional as HF
    a = torch.randn(12608, 40, device=DEV)
    assert HF.mm_wgrad_pays(a, torch.randn(12608, 24, device=DEV))
    assert not HF.mm_wgrad_pays(a[:160], torch.randn(160, 24, device=DEV))                 # a core contraction
    assert not HF.mm_wgrad_pays(torch.randn(40, 12608, device=DEV).t(), torch.randn(12608, 24, device=DEV))
    w = torch.randn(40, 24, device=DEV, requires_grad=True)
    g = torch.randn(12608, 24, device=DEV)
    HF.mm(a, w).backward(g)
    assert _rel(w.grad, a.double().t() @ g.double()) < 1e-5


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_device_untouched():
    from tadmm._cabi import TadmmError
    ops = _ops()
    a = torch.randn(64, 8, device=DEV)
    b = torch.randn(64, 6, device=DEV)
    img = torch.randn(2, 8, 4, 8, device=DEV)
    out = torch.full((8, 6), 7.0, device=DEV)
    bad = [
        (a.cpu(), b.cpu()), (a, b.cpu()),                       # host tensors
        (a, b.bfloat16()),                                      # mixed dtypes
        (img, b),                                               # mixed layouts
        (a, b[:63]),                                            # unequal T
        (img, torch.randn(2, 6, 8, 4, device=DEV)),             # unequal (H, W)
        (a.half(), b.half()),                                   # fp16
        (a.double(), b.double()),
    ]
    for x, y in bad:
        with pytest.raises(TadmmError):
            ops.wgrad(x, y, out=out)
    with pytest.raises(TadmmError):
        ops.wgrad(a, b, out=torch.empty(6, 8, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full((8, 6), 7.0, device=DEV))
    assert _rel(ops.wgrad(a, b, out=out, alpha=0.5), 0.5 * (a.double().t() @ b.double())) < 1e-5
