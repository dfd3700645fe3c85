"""Every instantiation of the training-side kernels against float64, ELEMENTWISE, at the smallest shapes that reach their
edges: the 36 `wgrad_kernel`s and the 18 `core_wgrad_kernel`s (csrc/wgrad.hip) with both epilogues (one slice writes C;
several slices go through the workspace and the fp64 reduce), the 6 `core_conv_kernel`s (csrc/coreconv.hip) as forward
and as data gradient, and every `tt_conv_kernel` (csrc/convchain.hip) that some descriptor reaches.  The case ids spell
the variant (`f32-rows-64x32-multi`, `bf16-core-16x64-one`, `f32-dgrad-nbw2`, `bf16-tm32-nbw4-5x5`).

The case tables, the rule that maps a case to its kernel and the criteria live in tests/_train_ref.py;
tests/test_train_ref_cpu.py shows without a GPU that the tables reach every variant and that the criteria discriminate.
Criteria: the derived elementwise bound of the dtype; for float32, and for bfloat16 weight gradients, also
rms(error) <= 2 x rms(error of the same operation in float32 by torch on the CPU); bitwise equality where two call forms
share a kernel (`out=` against allocate, aligned against offset operands, two runs, a NaN-filled workspace).

Measured on one MI355X (-s prints every figure; DESIGN.md section 26 has the table): worst share of the elementwise bound
0.008 / 0.045 / 0.003 / 0.037 for float32 wgrad / core wgrad / core convolution / conv chain and 0.63 - 0.66 for the 16-bit
convolutions; rms ratios 0.30 - 1.80, the largest being the `-fold` weight gradients.  Before `mma_tile_split`
(csrc/chain_common.h) the float32 conv chain failed the rms criterion at `f32-tm64-nbw4-3x3` (2.20) and
`f32-tm32-nbw4-3x3` (H2: 2.04); those cases are now at 0.91 and below.

Operands are Gaussian, factors scaled by fan_in^-1/2, cut out of sentinel-filled buffers at the offsets and row strides
that give each loader its three load widths; every output lies in a sentinel-guarded buffer."""
import ctypes as C
import functools
import gc

import pytest
import torch

import _train_ref as R
from _chain_ref import DTYPES, guarded, guards_intact, same_bits, untouched

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_INVALID, ERR_WORKSPACE = -1, -2


def _ops():
    from tadmm import ops
    return ops


def _lib():
    ops = _ops()
    h = ops.Handle.get(torch.cuda.current_device())
    return h, torch.cuda.current_stream().cuda_stream


def _placed(values, dtype, ld=None, off=0):
    """`values` as `dtype` inside a sentinel-filled buffer: row stride `ld`, first element `off` elements past 16 bytes."""
    v = guarded(tuple(values.shape), dtype, ld=ld, off=off)
    v.copy_(values.to(DEV).to(dtype))
    return v


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


@pytest.fixture(scope="module", autouse=True)
def _private_memory_pool():
    """Every device allocation of this module comes from a memory pool of its own, which goes back to the device when the
    module ends.  Later files measure the allocator (tests/test_gpu_wgrad.py::test_no_operand_copies asserts the peak of
    one launch, and a cached block of 5 MiB handed out for its 4 MiB workspace fails it): they must find torch's
    caching allocator exactly as if this file had not run -- neither the blocks its cases free nor an `empty_cache()`
    that drops what earlier files left."""
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        for cached in (_wgrad_operands, _core_wgrad_operands, _core_conv_operands, _conv_operands):
            cached.cache_clear()
        gc.collect()
    del pool


# =====================================================================================================================
# a. ops.wgrad: 36 kernels x {one slice, several slices}
# =====================================================================================================================
WGRAD = {c.id: c for c in R.WGRAD_CASES}


@functools.lru_cache(maxsize=4)
def _wgrad_operands(cid, aligned=False):
    """(a, b, ref, bound, plain32) of a case; `aligned`: the same values contiguous at 16-byte aligned bases."""
    c = WGRAD[cid]
    dtype = DTYPES[c.dn]
    g = torch.Generator().manual_seed(list(WGRAD).index(cid))
    if c.layout == "rows":
        va, vb = _randn(g, c.T, c.M), _randn(g, c.T, c.N)
        a = _placed(va, dtype, None if aligned else c.lda, 0 if aligned else c.offa)
        b = _placed(vb, dtype, None if aligned else c.ldb, 0 if aligned else c.offb)
    else:
        va, vb = _randn(g, c.B, c.M, *c.hw), _randn(g, c.B, c.N, *c.hw)
        a, b = _placed(va, dtype, off=0 if aligned else c.offa), _placed(vb, dtype, off=0 if aligned else c.offb)
    ref, bound = R.wgrad_bound(a, b, c.alpha, c.dn)
    return a, b, ref, bound, R.wgrad_plain32(a, b, c.alpha)


def _wgrad_abi(a, b, c, out, ws_fill=float("nan"), short=0):
    """`tadmm_wgrad` through the raw ABI into `out` (row stride out.stride(0)); returns (status, slices)."""
    ops = _ops()
    h, stream = _lib()
    hw = c.hw[0] * c.hw[1] if c.layout == "img" else 0
    d = ops._wgrad_desc(a, b, c.T, c.M, c.N, hw, c.alpha)
    nbytes, slices = C.c_size_t(), C.c_int()
    assert h.lib.tadmm_wgrad_workspace_bytes(C.byref(d), C.byref(nbytes), C.byref(slices)) == 0
    ws = torch.full((max(nbytes.value // 4, 4),), ws_fill, device=DEV)
    d.C, d.ldc = out.data_ptr(), out.stride(0)
    rc = h.lib.tadmm_wgrad(h.ptr, C.byref(d), ws.data_ptr(), nbytes.value - short, stream)
    torch.cuda.synchronize()
    return rc, slices.value


@pytest.mark.parametrize("cid", list(WGRAD))
def test_wgrad_variant(cid):
    ops = _ops()
    c = WGRAD[cid]
    a, b, ref, bound, plain = _wgrad_operands(cid)
    g = R.wgrad_geom(c.M, c.N, c.T)
    assert ops.wgrad_plan(a, b) == (g.ws_bytes, g.slices) and (g.TM, g.TN) == c.want[2:4]
    assert a.data_ptr() % 16 == c.offa * a.element_size() and b.data_ptr() % 16 == c.offb * b.element_size()
    out = guarded((c.M, c.N), torch.float32)
    assert ops.wgrad(a, b, out=out, alpha=c.alpha) is out
    assert guards_intact(out) and guards_intact(a) and guards_intact(b)
    R.judge(cid, out, ref, bound, plain, family=f"wgrad-{c.dn}")


@pytest.mark.parametrize("cid", ["f32-rows-32x64-one", "bf16-rows-64x16-multi", "f32-img-16x32-multi", "bf16-img-64x64-one"])
def test_wgrad_call_forms_share_bits(cid):
    """Allocate against `out=` at ldc > N through the raw ABI, and offset operands against aligned ones."""
    ops = _ops()
    c = WGRAD[cid]
    a, b, ref, bound, plain = _wgrad_operands(cid)
    first = ops.wgrad(a, b, alpha=c.alpha)
    wide = guarded((c.M, c.N), torch.float32, ld=c.N + 3)
    rc, slices = _wgrad_abi(a, b, c, wide)
    assert rc == 0 and slices == R.wgrad_geom(c.M, c.N, c.T).slices
    assert guards_intact(wide) and same_bits(wide, first)
    R.judge(cid + "-ldc", wide, ref, bound, plain, family=f"wgrad-{c.dn}")
    a2, b2, *_ = _wgrad_operands(cid, aligned=True)
    assert torch.equal(a2, a) and torch.equal(b2, b) and a2.data_ptr() % 16 == 0 and b2.data_ptr() % 16 == 0
    assert same_bits(ops.wgrad(a2, b2, alpha=c.alpha), first)


@pytest.mark.parametrize("cid", ["f32-rows-64x32-multi", "bf16-img-32x64-multi"])
def test_wgrad_abi_refusals_determinism_and_workspace(cid):
    c = WGRAD[cid]
    a, b, *_ = _wgrad_operands(cid)
    out = guarded((c.M, c.N), torch.float32)
    rc, slices = _wgrad_abi(a, b, c, out, short=1)                     # one byte short: nothing launched
    assert rc == ERR_WORKSPACE and slices > 1 and untouched(out) and guards_intact(out)
    narrow = guarded((c.M, c.N), torch.float32).as_strided((c.M, c.N), (c.N - 1, 1))
    assert _wgrad_abi(a, b, c, narrow)[0] == ERR_INVALID               # ldc < N
    assert bool((narrow._base == narrow._base[0]).all())
    runs = []
    for fill in (float("nan"), float("nan"), 0.0):
        o = guarded((c.M, c.N), torch.float32)
        assert _wgrad_abi(a, b, c, o, ws_fill=fill)[0] == 0 and guards_intact(o)
        runs.append(o)
    assert bool(torch.isfinite(runs[0]).all()) and same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2])


# =====================================================================================================================
# b. ops.core_conv_wgrad: 18 kernels x {one slice, several slices}
# =====================================================================================================================
CORE_WGRAD = {c.id: c for c in R.CORE_WGRAD_CASES}


@functools.lru_cache(maxsize=4)
def _core_wgrad_operands(cid):
    c = CORE_WGRAD[cid]
    dtype = DTYPES[c.dn]
    g = torch.Generator().manual_seed(100 + list(CORE_WGRAD).index(cid))
    ho, wo = R.out_hw(c.hw, c.k, c.s, c.p, c.dl)
    x = _placed(_randn(g, c.B, c.R1, *c.hw), dtype)
    dy = _placed(_randn(g, c.B, c.R2, ho, wo), dtype)
    ref, bound = R.core_wgrad_bound(dy, x, c.k, c.s, c.p, c.dl, c.dn)
    return x, dy, ref, bound, R.core_wgrad_plain32(dy, x, c.k, c.s, c.p, c.dl)


def _core_wgrad_abi(dy, x, geom, out, ws_fill=float("nan"), short=0, **over):
    """`tadmm_core_conv_wgrad` through the raw ABI into `out`; returns (status, slices)."""
    ops = _ops()
    h, stream = _lib()
    dy, x, d = ops._core_wgrad_operands(dy, x, *(R.pair(v) for v in geom))
    nbytes, slices = C.c_size_t(), C.c_int()
    assert h.lib.tadmm_core_conv_wgrad_workspace_bytes(C.byref(d), C.byref(nbytes), C.byref(slices)) == 0
    for name, v in over.items():
        setattr(d, name, v)
    ws = torch.full((max(nbytes.value // 4, 4),), ws_fill, device=DEV)
    rc = h.lib.tadmm_core_conv_wgrad(h.ptr, C.byref(d), out.data_ptr(), ws.data_ptr(), nbytes.value - short, stream)
    torch.cuda.synchronize()
    return rc, slices.value


@pytest.mark.parametrize("cid", list(CORE_WGRAD))
def test_core_wgrad_variant(cid):
    c = CORE_WGRAD[cid]
    x, dy, ref, bound, plain = _core_wgrad_operands(cid)
    want, g = R.core_wgrad_case_resolves(c)
    assert want == c.want
    assert _ops().core_conv_wgrad_plan(dy, x, R.pair(c.k), c.s, c.p, c.dl) == (g.ws_bytes, g.slices)
    out = guarded(tuple(ref.shape), torch.float32)
    rc, slices = _core_wgrad_abi(dy, x, (c.k, c.s, c.p, c.dl), out)
    assert rc == 0 and slices == g.slices
    assert guards_intact(out) and guards_intact(x) and guards_intact(dy)
    R.judge(cid, out, ref, bound, plain, family=f"core_wgrad-{c.dn}")


@pytest.mark.parametrize("cid", ["f32-core-64x64-multi", "bf16-core-32x64-multi"])
def test_core_wgrad_abi_refusals_determinism_and_workspace(cid):
    c = CORE_WGRAD[cid]
    x, dy, ref, *_ = _core_wgrad_operands(cid)
    geom = (c.k, c.s, c.p, c.dl)
    out = guarded(tuple(ref.shape), torch.float32)
    rc, slices = _core_wgrad_abi(dy, x, geom, out, short=1)
    assert rc == ERR_WORKSPACE and slices > 1 and untouched(out) and guards_intact(out)
    assert _core_wgrad_abi(dy, x, geom, out, Ho=c.hw[0] + 1)[0] == ERR_INVALID        # not the geometry's output plane
    assert untouched(out) and guards_intact(out)
    runs = []
    for fill in (float("nan"), float("nan"), 0.0):
        o = guarded(tuple(ref.shape), torch.float32)
        assert _core_wgrad_abi(dy, x, geom, o, ws_fill=fill)[0] == 0 and guards_intact(o)
        runs.append(o)
    assert bool(torch.isfinite(runs[0]).all()) and same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2])
    # the allocating call form and operands at an odd offset share the kernel
    first = _ops().core_conv_wgrad(dy, x, R.pair(c.k), c.s, c.p, c.dl)
    assert same_bits(first, runs[0])
    xo, dyo = _placed(x, x.dtype, off=1), _placed(dy, dy.dtype, off=1)
    assert same_bits(_ops().core_conv_wgrad(dyo, xo, R.pair(c.k), c.s, c.p, c.dl), first)


# =====================================================================================================================
# c. ops.core_conv and ops.core_conv_dgrad: 6 kernels x 2 directions
# =====================================================================================================================
CORE_CONV = {c.id: c for c in R.CORE_CONV_CASES}


def _core_conv_shapes(c):
    """(x_shape, r2, source shape, destination shape)."""
    r1, r2 = (c.src, c.dst) if c.direction == "fwd" else (c.dst, c.src)
    x_shape = (c.B, r1, *c.hw)
    y_shape = (c.B, r2, *R.out_hw(c.hw, c.k, c.s, c.p, c.dl))
    return (x_shape, r2) + ((x_shape, y_shape) if c.direction == "fwd" else (y_shape, x_shape))


@functools.lru_cache(maxsize=4)
def _core_conv_operands(cid):
    c = CORE_CONV[cid]
    ops = _ops()
    dtype = DTYPES[c.dn]
    x_shape, r2, s_shape, d_shape = _core_conv_shapes(c)
    g = torch.Generator().manual_seed(200 + list(CORE_CONV).index(cid))
    src = _placed(_randn(g, *s_shape), dtype, off=R.align_offset(c.dn, c.align))
    core = (_randn(g, r2, x_shape[1], c.k, c.k) * (x_shape[1] * c.k * c.k) ** -0.5).to(DEV)
    nplanes = 3 if c.dn == "f32" else 1
    if nplanes == 1:
        core = core.bfloat16().float()                                  # the one plane the kernel multiplies with
    planes = ops.conv_core_planes(core if c.direction == "fwd" else core.permute(1, 0, 2, 3), nplanes)
    steps = R.core_conv_steps(core, c.direction, c.hw, c.s, c.p, c.dl)
    (ref, bound), = R.prefix_bounds(src, steps, c.dn)
    plain = R.prefix_plain32(src, steps)[0] if c.dn == "f32" else None
    return src, planes, ref, bound, plain


def _core_conv_abi(c, src, planes, out, **over):
    ops = _ops()
    h, stream = _lib()
    x_shape, r2, _, _ = _core_conv_shapes(c)
    d = ops._core_conv_desc(x_shape, r2, src.dtype, c.k, c.s, c.p, c.dl)
    d.Wc, d.wc_plane = planes.data_ptr(), planes[0].numel()
    d.X, d.Y = (src.data_ptr(), out.data_ptr()) if c.direction == "fwd" else (out.data_ptr(), src.data_ptr())
    for name, v in over.items():
        setattr(d, name, v)
    entry = h.lib.tadmm_core_conv_fwd if c.direction == "fwd" else h.lib.tadmm_core_conv_dgrad
    rc = entry(h.ptr, C.byref(d), stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("cid", list(CORE_CONV))
def test_core_conv_variant(cid):
    ops = _ops()
    c = CORE_CONV[cid]
    src, planes, ref, bound, plain = _core_conv_operands(cid)
    assert R.align_class(src.data_ptr() % 16) == c.align
    x_shape, r2, _, d_shape = _core_conv_shapes(c)
    out = guarded(d_shape, src.dtype)
    assert _core_conv_abi(c, src, planes, out) == 0
    assert guards_intact(out) and guards_intact(src)
    R.judge(cid, out, ref, bound, plain, family=f"core_conv-{c.dn}")
    # the allocating call form on an aligned copy of the source shares the kernel
    aligned = src.clone()
    assert aligned.data_ptr() % 16 == 0
    geom = ((c.k, c.k), c.s, c.p, c.dl)
    if c.direction == "fwd":
        again = ops.core_conv(aligned, planes, r2, *geom, memo=False)
    else:
        again = ops.core_conv_dgrad(aligned, planes, x_shape, *geom, memo=False)
    assert same_bits(again, out)


def test_core_conv_abi_refusal_and_determinism():
    for cid in ("f32-fwd-nbw2", "bf16-dgrad-nbw4"):
        c = CORE_CONV[cid]
        src, planes, *_ = _core_conv_operands(cid)
        d_shape = _core_conv_shapes(c)[3]
        out = guarded(d_shape, src.dtype)
        assert _core_conv_abi(c, src, planes, out, Wo=1) == ERR_INVALID           # not the geometry's output plane
        assert _core_conv_abi(c, src, planes, out, wc_plane=512) == ERR_INVALID   # planes too small for the ranks
        assert untouched(out) and guards_intact(out)
        one, two = guarded(d_shape, src.dtype), guarded(d_shape, src.dtype)
        assert _core_conv_abi(c, src, planes, one) == 0 and _core_conv_abi(c, src, planes, two) == 0
        assert same_bits(one, two)


# =====================================================================================================================
# d. the one-launch factorised convolution: every reachable (dtype, TM, NBW, mode)
# =====================================================================================================================
CONV = {c.id: c for c in R.CONV_CHAIN_CASES}


@functools.lru_cache(maxsize=2)
def _conv_operands(cid):
    """Operands scaled as in tests/test_gpu_conv_chain_train.py, the planes of both directions, and (ref, bound, plain32)
    of Y, H1, H2, dX, dH1, dH2 for the values the kernels multiply (the weights rounded into their one plane)."""
    ops = _ops()
    c = CONV[cid]
    dtype = DTYPES[c.dn]
    k = R.pair(c.k)
    g = torch.Generator().manual_seed(300 + list(CONV).index(cid))
    x = _placed(_randn(g, 2, c.C, *c.hw), dtype)
    w1 = (_randn(g, c.r1, c.C) * c.C ** -0.5).to(DEV)
    core = (_randn(g, c.r2, c.r1, *k) * (c.r1 * k[0] * k[1]) ** -0.5).to(DEV)
    w3 = (_randn(g, c.O, c.r2) * c.r2 ** -0.5).to(DEV)
    bias = _randn(g, c.O).to(DEV)
    ho, wo = R.out_hw(c.hw, c.k, c.s, c.p, c.dl)
    dy = _placed(_randn(g, 2, c.O, ho, wo), dtype)
    n, pdt = (3, torch.bfloat16) if c.dn == "f32" else (1, dtype)
    if n == 1:
        w1, core, w3 = (t.to(dtype).float() for t in (w1, core, w3))
    fwd = (ops.weight_planes(w1, n, pad_rows=32, dtype=pdt), ops.conv_core_planes(core, n, dtype=pdt), ops.weight_planes(w3, n, dtype=pdt))
    bwd = (ops.weight_planes(w3.t(), n, pad_rows=32, dtype=pdt), ops.conv_core_planes(core.permute(1, 0, 2, 3), n, dtype=pdt),
           ops.weight_planes(w1.t(), n, dtype=pdt))
    steps_f, steps_b = R.chain_steps(w1, core, w3, c.hw, c.s, c.p, c.dl)
    f32 = c.dn == "f32"
    refs = {}
    plain = R.prefix_plain32(x, steps_f, bias) if f32 else [None] * 3
    for name, (ref, bound), pl in zip(("h1", "h2", "y"), R.prefix_bounds(x, steps_f, c.dn, bias), plain):
        refs[name] = (ref, bound, pl)
    plain = R.prefix_plain32(dy, steps_b) if f32 else [None] * 3
    for name, (ref, bound), pl in zip(("dh2", "dh1", "dx"), R.prefix_bounds(dy, steps_b, c.dn), plain):
        refs[name] = (ref, bound, pl)
    # a pixel of H1 that no tap of any output pixel reads is stored as zero
    reach = R.reached(c.hw, c.k, c.s, c.p, c.dl, DEV)
    ref, bound, pl = refs["h1"]
    refs["h1"] = (ref * reach, bound * reach, None if pl is None else pl * reach.cpu())
    return x, dy, bias, fwd, bwd, refs, reach


@pytest.mark.parametrize("cid", list(CONV))
def test_conv_chain_variant(cid):
    ops = _ops()
    c = CONV[cid]
    dtype = DTYPES[c.dn]
    x, dy, bias, fwd, bwd, refs, reach = _conv_operands(cid)
    geom = tuple(R.pair(v) for v in (c.k, c.s, c.p, c.dl))
    reaches = R.conv_chain_case_resolves(c, lib=True)
    assert reaches == R.conv_chain_case_resolves(c) and "fwd" in reaches
    family = f"conv_chain-{c.dn}"
    ho, wo = R.out_hw(c.hw, *geom)
    shapes_f = ((2, c.O, ho, wo), (2, c.r1, *c.hw), (2, c.r2, ho, wo))
    shapes_b = (tuple(x.shape), shapes_f[1], shapes_f[2])
    got = {}
    y = guarded(shapes_f[0], dtype)
    assert ops.conv_chain(x, *fwd, bias, c.O, *geom, memo=False, out=y) is y
    assert guards_intact(y) and guards_intact(x)
    R.judge(f"{cid} fwd y", y, *refs["y"], family=family)
    if "fwd_save" in reaches:
        outs = tuple(guarded(s, dtype) for s in shapes_f)
        ops.conv_chain_save(x, *fwd, bias, c.O, c.r1, c.r2, *geom, out=outs)
        assert all(guards_intact(t) for t in outs) and guards_intact(x)
        for name, t in zip(("y", "h1", "h2"), outs):
            got[name] = t
            R.judge(f"{cid} fwd_save {name}", t, *refs[name], family=family)
        assert float(got["h1"][:, :, ~reach].abs().max() if bool((~reach).any()) else 0.0) == 0.0
    if "bwd" in reaches:
        dx = guarded(shapes_b[0], dtype)
        ops.conv_chain_bwd(dy, *bwd, x.shape, c.r1, c.r2, *geom, out=dx)
        assert guards_intact(dx) and guards_intact(dy)
        R.judge(f"{cid} bwd dx", dx, *refs["dx"], family=family)
        outs = tuple(guarded(s, dtype) for s in shapes_b)
        ops.conv_chain_bwd(dy, *bwd, x.shape, c.r1, c.r2, *geom, save=True, out=outs)
        assert all(guards_intact(t) for t in outs) and guards_intact(dy)
        for name, t in zip(("dx", "dh1", "dh2"), outs):
            got[name] = t
            R.judge(f"{cid} bwd_save {name}", t, *refs[name], family=family)
        if bool((~reach).any()):
            assert float(got["dx"][:, :, ~reach].abs().max()) == 0.0
    if len(got) == 6:
        # the three weight gradients, against the float64 products of the tensors their kernels read
        dn = c.dn
        for name, a, b in (("dw3", dy, got["h2"]), ("dw1", got["dh1"], x)):
            ref, bound = R.wgrad_bound(a, b, 1.0, dn)
            R.judge(f"{cid} {name}", ops.wgrad(a, b), ref, bound, R.wgrad_plain32(a, b, 1.0), family=f"wgrad-{dn}")
        ref, bound = R.core_wgrad_bound(got["dh2"], got["h1"], *geom, dn)
        R.judge(f"{cid} dwc", ops.core_conv_wgrad(got["dh2"], got["h1"], *geom), ref, bound,
                R.core_wgrad_plain32(got["dh2"], got["h1"], *geom), family=f"core_wgrad-{dn}")
    else:
        assert c.dn == "f16" or "bwd" not in reaches, (cid, sorted(got))


def test_conv_chain_abi_refusal_and_determinism():
    from tadmm import ops
    for cid in ("f32-tm64-nbw2-3x3", "bf16-tm64-nbw4-1x1s2"):
        c = CONV[cid]
        dtype = DTYPES[c.dn]
        x, dy, bias, fwd, bwd, refs, reach = _conv_operands(cid)
        geom = tuple(R.pair(v) for v in (c.k, c.s, c.p, c.dl))
        ho, wo = R.out_hw(c.hw, *geom)
        h, stream = _lib()
        y, h1, h2 = guarded((2, c.O, ho, wo), dtype), guarded((2, c.r1, *c.hw), dtype), guarded((2, c.r2, ho, wo), dtype)
        dx = guarded(tuple(x.shape), dtype)
        P = lambda t: C.c_void_p(t.data_ptr())                                  # noqa: E731

        def desc(planes, src, dst, backward=False, **over):
            d, _, _ = ops._conv_chain_desc(2, c.C, *c.hw, c.O, *planes, None, dtype, *geom, bwd=backward)
            d.X, d.Y = src.data_ptr(), dst.data_ptr()
            for name, v in over.items():
                setattr(d, name, v)
            return d

        lib = h.lib
        assert lib.tadmm_ttconv_fused(h.ptr, C.byref(desc(fwd, x, y, Ho=ho + 1)), stream) == ERR_INVALID
        assert lib.tadmm_ttconv_fused_save(h.ptr, C.byref(desc(fwd, x, y)), c.r1, 0, P(h1), P(h2), stream) == ERR_INVALID
        assert lib.tadmm_ttconv_fused_bwd(h.ptr, C.byref(desc(bwd, dy, dx, True)), c.r1, c.r2, P(h1), None, stream) == ERR_INVALID
        torch.cuda.synchronize()
        for t in (y, h1, h2, dx):
            assert untouched(t) and guards_intact(t)
        runs = []
        for _ in range(2):
            outs_f = tuple(guarded(tuple(t.shape), dtype) for t in (y, h1, h2))
            outs_b = tuple(guarded(tuple(t.shape), dtype) for t in (dx, h1, h2))
            ops.conv_chain_save(x, *fwd, bias, c.O, c.r1, c.r2, *geom, out=outs_f)
            ops.conv_chain_bwd(dy, *bwd, x.shape, c.r1, c.r2, *geom, save=True, out=outs_b)
            runs.append(outs_f + outs_b)
        for a, b in zip(*runs):
            assert same_bits(a, b)


def test_print_the_worst_figures():
    """Last in the file: the worst bound ratio and rms ratio of every family and dtype (shown with -s)."""
    for family, (worst, ratio) in sorted(R.FIGURES.items()):
        print(f"train figures {family}: worst err / bound {worst:.4f}, worst rms ratio {ratio:.3f}")
