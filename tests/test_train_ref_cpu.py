"""The case tables and yardsticks of tests/test_gpu_train_variants.py, checked without a GPU.

(a) Coverage: every case of the four tables resolves -- by the Python restatement of the host rule in tests/_train_ref.py
and, where a host-only query exists, by the library's own answer -- to the variant it is meant to reach, and the tables
reach every variant of their target sets.  Removing a case from a table fails one of these tests.

(b) Discrimination: the CPU models of tests/_chain_ref.py pass every criterion at the shapes of the GPU tables as built,
and fail the rms criterion with any one of the six kept plane pairs dropped.  Figures (printed with -s): see the section
on these files in DESIGN.md."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import _train_ref as R
from _chain_ref import DTYPES, KEPT_PAIRS, half_chain_model, three_plane_chain, three_plane_emulation
from _fp16_ref import conv_bound


# ------------------------------------------------------------------------------------------------ (a) coverage
def _wgrad_lib(c):
    """(workspace bytes, slices) of a weight-gradient case from `tadmm_wgrad_workspace_bytes` (host only)."""
    from tadmm import _cabi
    d = _cabi.WgradDesc()
    esz = R.ESZ[c.dn]
    d.A, d.B = 4096 + c.offa * esz, 8192 + c.offb * esz           # never read: the query looks at shapes and alignment
    d.T, d.M, d.N = c.T, c.M, c.N
    d.hw = c.hw[0] * c.hw[1] if c.layout == "img" else 0
    d.lda, d.ldb = c.lda, c.ldb
    d.dtype = _cabi.CHAIN_F32 if c.dn == "f32" else _cabi.CHAIN_BF16
    d.alpha = 1.0
    nbytes, slices = C.c_size_t(), C.c_int()
    assert _cabi.load().tadmm_wgrad_workspace_bytes(C.byref(d), C.byref(nbytes), C.byref(slices)) == 0
    return nbytes.value, slices.value


def test_wgrad_table_reaches_all_36_kernels_with_both_epilogues():
    seen, loaders, folds = set(), set(), set()
    for c in R.WGRAD_CASES:
        variant, va, vb, chunks = R.wgrad_case_resolves(c)
        assert variant == c.want, (c.id, variant)
        g = R.wgrad_geom(c.M, c.N, c.T)
        nbytes, slices = _wgrad_lib(c)
        assert slices == g.slices, (c.id, slices, g)
        assert nbytes == (slices * g.tiles * g.TM * g.TN * 4 if slices > 1 else 0) == g.ws_bytes, (c.id, nbytes, g)
        seen.add(variant)
        loaders.add((c.dn, c.layout, g.TM, va))
        loaders.add((c.dn, c.layout, g.TN, vb))
        if max(chunks) > R.WG_FOLD:
            folds.add((c.dn, c.layout))
        if c.id.endswith("-one") or c.id.endswith("-multi"):
            want_chunks = [2, 3, 2, 3] if variant[4] == "multi" else [3]
            assert chunks == want_chunks and c.T % R.WG_KC in (5, 9, 32, 36, 64), (c.id, chunks, c.T)    # a ragged last chunk
            assert _ceil(c.M, g.TM) * g.TM != c.M and _ceil(c.N, g.TN) * g.TN != c.N                    # ragged last tiles
    missing = {v + (e,) for v in R.WGRAD_VARIANTS for e in ("one", "multi")} - seen
    assert not missing, sorted(missing)
    # each of the 12 loaders (F x dtype x layout) at 16-byte, 8-byte and element loads, as operand A or B
    want = {(dn, lay, f, v) for dn in ("f32", "bf16") for lay in ("rows", "img") for f in R.TILES for v in (0, 1, 2)}
    assert not want - loaders, sorted(want - loaders)
    assert folds == {(dn, lay) for dn in ("f32", "bf16") for lay in ("rows", "img")}, folds
    # the row loader's (t, t + 1) pair ends on a token that does not exist: an odd T
    assert R.T_ONE % 2 == 1 and R.T_ONE % R.WG_KC == 5


def _ceil(a, b):
    return -(-a // b)


def _core_desc(dn, x_shape, r2, k, s, p, dl):
    from tadmm import ops
    d = ops._core_conv_desc(tuple(x_shape), r2, DTYPES[dn], k, s, p, dl)
    d.X, d.Y = 4096, 8192                                          # never read by the host-only query
    return d


def test_core_wgrad_table_reaches_all_18_kernels_with_both_epilogues():
    from tadmm import _cabi
    seen = set()
    for c in R.CORE_WGRAD_CASES:
        variant, g = R.core_wgrad_case_resolves(c)
        assert variant == c.want, (c.id, variant)
        d = _core_desc(c.dn, (c.B, c.R1, *c.hw), c.R2, c.k, c.s, c.p, c.dl)
        nbytes, slices = C.c_size_t(), C.c_int()
        assert _cabi.load().tadmm_core_conv_wgrad_workspace_bytes(C.byref(d), C.byref(nbytes), C.byref(slices)) == 0
        taps = R.pair(c.k)[0] * R.pair(c.k)[1]
        assert slices.value == g.slices, (c.id, slices.value, g)
        assert nbytes.value == (taps * g.slices * g.tiles * g.TM * g.TN * 4 if g.slices > 1 else 0) == g.ws_bytes, (c.id, g)
        if variant[3] == "multi":
            ho, wo = R.out_hw(c.hw, c.k, c.s, c.p, c.dl)
            assert c.B * ho * wo == 512
        seen.add(variant)
    missing = {v + (e,) for v in R.CORE_WGRAD_VARIANTS for e in ("one", "multi")} - seen
    assert not missing, sorted(missing)
    # the two float32 tiles above 64 KiB of LDS (the dynamic-LDS opt-in): 64 x 64 needs 104 KiB, 64 x 32 / 32 x 64 78 KiB
    lds = lambda planes, tm, tn: planes * (tm + tn) * (R.WG_KC + 8) * 2                       # noqa: E731
    assert lds(3, 64, 64) == 104448 and lds(3, 64, 32) == 78336 and lds(3, 32, 32) <= 64 * 1024 and lds(1, 64, 64) <= 64 * 1024


def test_core_conv_table_reaches_all_6_kernels_in_both_directions():
    seen, aligns = set(), set()
    for c in R.CORE_CONV_CASES:
        assert (c.dn, R.cc_nbw(c.dst), c.direction) == c.want, c.id
        assert R.align_class(R.align_offset(c.dn, c.align) * R.ESZ[c.dn]) == c.align
        kc = 32 if c.dn == "f32" else 64
        assert c.src % kc != 0                                      # a ragged chunk of source channels
        seen.add(c.want)
        aligns.add((c.dn, c.align))
    assert seen == {v + (d,) for v in R.CORE_CONV_VARIANTS for d in ("fwd", "dgrad")}
    assert aligns == {(dn, a) for dn in ("f32", "bf16") for a in (0, 1, 2)}
    assert {c.src for c in R.CORE_CONV_CASES} == set(R.CC_SRC)


def test_conv_chain_table_reaches_every_reachable_instantiation():
    targets = R.conv_chain_targets()
    unreachable = sorted(set(R.CONV_CHAIN_VARIANTS) - targets)
    print(f"conv chain: {len(targets)} of {len(R.CONV_CHAIN_VARIANTS)} instantiations reachable; unreachable:")
    for v in unreachable:
        print("   ", v)
    for key, (plane, k, s, r1, r2) in sorted(R.conv_chain_reachable().items()):
        print(f"    first reached {key}: plane {plane}, kernel {k}, stride {s}, padded ranks ({r1}, {r2})")
    assert targets <= set(R.CONV_CHAIN_VARIANTS)
    seen = set()
    for c in R.CONV_CHAIN_CASES:
        by_rule, by_lib = R.conv_chain_case_resolves(c), R.conv_chain_case_resolves(c, lib=True)
        assert by_rule == by_lib, (c.id, by_rule, by_lib)
        assert "fwd" in by_rule, c.id
        assert c.r1 % 16 and c.r2 % 16 and c.C % 16 and c.O % 16     # ragged everything
        print(f"    {c.id}: " + ", ".join(f"{m} -> TM {v[1]} NBW {v[2]}" for m, v in by_rule.items()))
        seen |= set(by_rule.values())
    assert not targets - seen, sorted(targets - seen)
    # known to be reachable by reading plan_tt_conv, at least
    for dn in ("f32", "bf16"):
        for nbw in (1, 2, 4):
            assert {(dn, 64, nbw, "fwd"), (dn, 64, nbw, "bwd")} <= targets
    assert {("f32", 32, 1, "fwd"), ("f32", 32, 2, "fwd"), ("f32", 32, 4, "fwd"), ("f32", 32, 2, "bwd"), ("f32", 32, 4, "bwd"),
            ("bf16", 32, 4, "fwd")} <= targets


def test_no_case_has_left_a_table():
    """The single-tile, fold, alpha and 5 x 5 cases reach variants other cases reach too: their count pins them."""
    assert (len(R.WGRAD_CASES), len(R.CORE_WGRAD_CASES), len(R.CORE_CONV_CASES), len(R.CONV_CHAIN_CASES)) == (90, 38, 12, 30)
    for table in (R.WGRAD_CASES, R.CORE_WGRAD_CASES, R.CORE_CONV_CASES, R.CONV_CHAIN_CASES):
        assert len({c.id for c in table}) == len(table)


def test_the_restated_rules_on_known_values():
    assert [R.wgrad_tile(m) for m in (9, 23, 50, 40, 89, 120, 1000, 1010)] == [16, 32, 64, 16, 32, 64, 64, 64]
    assert R.wgrad_geom(40, 89, 261) == R.Geom(16, 32, 9, 1, 3, 0)
    assert R.slice_chunks(R.wgrad_geom(40, 89, 1157)) == [2, 3, 2, 3]
    assert R.slice_chunks(R.wgrad_geom(*R.FOLD_MN, R.T_FOLD)) == [9, 10]
    assert [R.cc_nbw(n) for n in (1, 64, 65, 128, 129, 264)] == [1, 1, 2, 2, 4, 4]
    assert [R.wgrad_vec(o, st, 4) for o, st in ((0, 36, ), (8, 36), (4, 36), (0, 9), (0, 18))] == [2, 1, 0, 0, 1]
    assert [R.wgrad_vec(o, st, 2) for o, st in ((0, 64), (0, 36), (8, 64), (2, 64), (0, 9))] == [2, 1, 1, 0, 0]


# ------------------------------------------------------------------------------------------------ (b) discrimination
def _wgrad_shapes():
    """The distinct (M, N, T) of the float32 weight-gradient cases (both layouts share the arithmetic)."""
    shapes = []
    for c in R.WGRAD_CASES:
        if c.dn == "f32" and c.alpha == 1.0 and (c.M, c.N, c.T) not in shapes:
            shapes.append((c.M, c.N, c.T))
    return shapes


_WG = {}


def _wgrad_operands(shape):
    if shape not in _WG:
        M, N, T = shape
        g = torch.Generator().manual_seed(M + 3 * N + T)
        a, b = torch.randn(T, M, generator=g), torch.randn(T, N, generator=g)
        _WG[shape] = (a, b, R.wgrad_bound(a, b, 1.0, "f32"), R.wgrad_plain32(a, b, 1.0))
    return _WG[shape]


def _figures(y, ref, bound, plain):
    err = (y.double() - ref).abs()
    return (err / bound).max().item(), R.rms_ratio(y, ref, plain)


@pytest.mark.parametrize("shape", _wgrad_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_weight_gradient_model_passes_and_every_dropped_pair_fails_the_rms_criterion(shape):
    a, b, (ref, bound), plain = _wgrad_operands(shape)
    worst, ratio = _figures(three_plane_emulation(a.t().contiguous(), b.t().contiguous()), ref, bound, plain)
    print(f"wgrad model {shape}: intact worst err / bound {worst:.4f}, rms ratio {ratio:.3f}")
    assert worst <= 1.0 and ratio <= 2.0
    for drop in KEPT_PAIRS:
        w, r = _figures(three_plane_emulation(a.t().contiguous(), b.t().contiguous(), drop=drop), ref, bound, plain)
        print(f"wgrad model {shape} without {drop}: worst err / bound {w:.3f}, rms ratio {r:.2f}")
        assert r > 2.0, (drop, r)


def test_bfloat16_weight_gradient_model_passes_both_criteria():
    """bfloat16 operands: one plane, exact products; the model is a float32 matmul in another order."""
    for shape in ((40, 89, 261), (120, 120, 1157)):
        a, b = (t.bfloat16() for t in _wgrad_operands(shape)[:2])
        ref, bound = R.wgrad_bound(a, b, 1.0, "bf16")
        plain = R.wgrad_plain32(a, b, 1.0)
        y = torch.zeros_like(plain)
        for t0 in range(0, a.shape[0], 32):                         # k-steps of 32 tokens, as the MFMA accumulates
            y = y + a[t0:t0 + 32].float().t() @ b[t0:t0 + 32].float()
        worst, ratio = _figures(y, ref, bound, plain)
        print(f"wgrad bf16 model {shape}: worst err / bound {worst:.4f}, rms ratio {ratio:.3f}")
        assert worst <= 1.0 and ratio <= 2.0


def _core_conv_shapes():
    shapes = []
    for c in R.CORE_CONV_CASES:
        if c.dn == "f32" and c.direction == "fwd":
            shapes.append((c.src, c.dst, c.B, c.hw, c.k, c.s, c.p, c.dl))
    return shapes


@pytest.mark.parametrize("shape", _core_conv_shapes(), ids=lambda s: f"{s[0]}to{s[1]}-{s[3][0]}x{s[3][1]}-s{s[5]}")
def test_core_convolution_model_passes_and_every_dropped_pair_fails_the_rms_criterion(shape):
    r1, r2, B, hw, k, s, p, dl = shape
    g = torch.Generator().manual_seed(r1 + r2)
    x = torch.randn(B, r1, *hw, generator=g)
    core = torch.randn(r2, r1, k, k, generator=g) * (r1 * k * k) ** -0.5
    steps = R.core_conv_steps(core, "fwd", hw, s, p, dl)
    (ref, bound), = R.prefix_bounds(x, steps, "f32")
    plain, = R.prefix_plain32(x, steps)
    ho, wo = R.out_hw(hw, k, s, p, dl)
    as_image = lambda y: y.reshape(B, ho, wo, r2).permute(0, 3, 1, 2)                          # noqa: E731
    rows, wmat = R.unfold_rows(x, k, s, p, dl), core.reshape(r2, -1)
    worst, ratio = _figures(as_image(three_plane_emulation(rows, wmat)), ref, bound, plain)
    print(f"core conv model {shape}: intact worst err / bound {worst:.4f}, rms ratio {ratio:.3f}")
    assert worst <= 1.0 and ratio <= 2.0
    for drop in KEPT_PAIRS:
        w, r = _figures(as_image(three_plane_emulation(rows, wmat, drop=drop)), ref, bound, plain)
        print(f"core conv model {shape} without {drop}: worst err / bound {w:.3f}, rms ratio {r:.2f}")
        assert r > 2.0, (drop, r)
    # bfloat16: the one-plane model of the same product stays inside its bound
    y16, xq, wq = half_chain_model(rows, [wmat], None, torch.bfloat16)
    (ref16, bound16), = R.prefix_bounds(x.bfloat16(), R.core_conv_steps(wq[0].float().reshape(core.shape), "fwd", hw, s, p, dl), "bf16")
    assert bool(((as_image(y16).double() - ref16).abs() <= bound16).all())


def _chain_1x1_shapes():
    """The 1 x 1-core cases of the conv-chain table: pure three-factor chains on the pixels the stride keeps."""
    return [(c.id, c.C, c.O, c.r1, c.r2, c.hw, c.s) for c in R.CONV_CHAIN_CASES if c.dn == "f32" and R.pair(c.k) == (1, 1)]


@pytest.mark.parametrize("shape", _chain_1x1_shapes(), ids=lambda s: s[0])
def test_conv_chain_model_passes_and_every_dropped_pair_fails_the_rms_criterion(shape):
    _, C_, O, r1, r2, hw, s = shape
    g = torch.Generator().manual_seed(C_ + r1 + r2)
    x = torch.randn(2, C_, *hw, generator=g)
    w1 = torch.randn(r1, C_, generator=g) * C_ ** -0.5
    core = torch.randn(r2, r1, 1, 1, generator=g) * r1 ** -0.5
    w3 = torch.randn(O, r2, generator=g) * r2 ** -0.5
    bias = torch.randn(O, generator=g)
    fwd, _ = R.chain_steps(w1, core, w3, hw, s, 0, 1)
    ref, bound = R.prefix_bounds(x, fwd, "f32", bias)[-1]
    plain = R.prefix_plain32(x, fwd, bias)[-1]
    xs = x[:, :, ::s, ::s]
    rows = xs.permute(0, 2, 3, 1).reshape(-1, C_)
    as_image = lambda y: y.reshape(2, xs.shape[2], xs.shape[3], O).permute(0, 3, 1, 2)         # noqa: E731
    ws = [w1, core[:, :, 0, 0], w3]
    worst, ratio = _figures(as_image(three_plane_chain(rows, ws, bias)), ref, bound, plain)
    print(f"conv chain model {shape}: intact worst err / bound {worst:.4f}, rms ratio {ratio:.3f}")
    assert worst <= 1.0 and ratio <= 2.0
    for drop in KEPT_PAIRS:
        w, r = _figures(as_image(three_plane_chain(rows, ws, bias, drop=drop)), ref, bound, plain)
        print(f"conv chain model {shape} without {drop}: worst err / bound {w:.3f}, rms ratio {r:.2f}")
        assert r > 2.0, (drop, r)
    for dtype, dn in ((torch.bfloat16, "bf16"), (torch.float16, "f16")):
        y16, xq, wq = half_chain_model(rows, ws, bias, dtype)
        steps16, _ = R.chain_steps(wq[0].float(), wq[1].float()[:, :, None, None], wq[2].float(), hw, s, 0, 1)
        ref16, bound16 = R.prefix_bounds(x.to(dtype), steps16, dn, bias)[-1]
        assert bool(((as_image(y16).double() - ref16).abs() <= bound16).all()), dn


def test_prefix_bounds_are_conv_bound_and_linear_bound_f32():
    """The generic prefix bound reproduces `conv_bound` of _fp16_ref.py (three products, 16-bit) and the n + 5 of
    `linear_bound_f32` (two products, float32): nothing is re-derived."""
    from _chain_ref import linear_bound_f32
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 24, 9, 8, generator=g)
    w1, core, w3 = torch.randn(20, 24, generator=g), torch.randn(28, 20, 3, 3, generator=g), torch.randn(40, 28, generator=g)
    bias = torch.randn(40, generator=g)
    fwd, bwd = R.chain_steps(w1, core, w3, (9, 8), 2, 1, 1)
    for dtype, dn in ((torch.bfloat16, "bf16"), (torch.float16, "f16")):
        ref, bound = conv_bound(x, w1, core, w3, bias, 2, 1, 1, dtype)
        got = R.prefix_bounds(x, fwd, dn, bias)
        assert torch.equal(got[-1][0], ref) and torch.allclose(got[-1][1], bound, rtol=1e-12, atol=0)
    xr = torch.randn(33, 24, generator=g)
    two = [(lambda t, w: t @ w.t(), w1, 24), (lambda t, w: t @ w.t(), torch.randn(40, 20, generator=g), 20)]
    ref, bound = linear_bound_f32(xr, [two[0][1], two[1][1]], bias)
    got = R.prefix_bounds(xr, two, "f32", bias)
    assert torch.equal(got[-1][0], ref) and torch.allclose(got[-1][1], bound, rtol=1e-12, atol=0)
    # the data-gradient steps are the autograd of the forward steps
    x64 = x.double().requires_grad_()
    y = F.conv2d(F.conv2d(F.conv2d(x64, w1.double()[:, :, None, None]), core.double(), None, 2, 1, 1), w3.double()[:, :, None, None])
    dy = torch.randn(y.shape, generator=g)
    dx, = torch.autograd.grad(y, x64, dy.double())
    assert torch.allclose(R.prefix_bounds(dy, bwd, "f32")[-1][0], dx, rtol=1e-12, atol=1e-12)
    miss = ~R.reached((8, 8), 1, 2, 0, 1)
    assert int(miss.sum()) == 48


def test_core_wgrad_reference_is_the_autograd_of_the_convolution():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 5, 9, 8, generator=g, dtype=torch.float64)
    core = torch.randn(7, 5, 3, 3, generator=g, dtype=torch.float64).requires_grad_()
    for s, p, dl in ((2, 1, 1), (1, 2, 2)):
        y = F.conv2d(x, core, None, s, p, dl)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        dw, = torch.autograd.grad(y, core, dy)
        ref, bound = R.core_wgrad_bound(dy, x, 3, s, p, dl, "f32")
        assert torch.allclose(ref, dw, rtol=1e-12, atol=1e-12) and bool((bound > 0).all())
        dx, = torch.autograd.grad(F.conv2d(xr := x.clone().requires_grad_(), core.detach(), None, s, p, dl), xr, dy)
        (ref, _), = R.prefix_bounds(dy, R.core_conv_steps(core.detach(), "dgrad", (9, 8), s, p, dl), "f32")
        assert torch.allclose(ref, dx, rtol=1e-12, atol=1e-12)
