"""Projection sweeps (unfold, fold/update, residual) and the ADMM penalty on operands a fresh torch allocation never
produces: W / U / Z whose base pointer is only 4-byte aligned (a contiguous view into a flat parameter buffer),
conv layers whose input channels span several chunks of the sweep kernels, and penalty layer tables whose
concatenated offsets are odd.

What the kernels choose from the pointer (csrc/sweep_kernels.hip): the float4 body of the flat (K2 == 1) unfold and
fold, `conv_vec_ok()` of the 3x3 transposes, the aligned middle of `penalty_kernel`.  Every check here is either
bitwise (fp32 add / subtract / copy have one result), an fp64 sum up to its summation order (n * 2^-52), or the
oracle bar of tests/test_gpu_projection.py::test_ragged_shapes_and_edge_ranks_vs_oracle (2e-5 * max|W + U|).

Measured on MI355X: two plan INSTANCES over the same data (one aligned, one misaligned) give bitwise equal Z and U
and residuals within n * 2^-52 in every combination below; the twin assertions are kept bitwise."""
import numpy as np
import pytest
import torch

from oracle import tt_oracle as O

pytestmark = pytest.mark.gpu

BAR = 2e-5                       # of max|W + U|: the bar of test_ragged_shapes_and_edge_ranks_vs_oracle
EPS64 = 2.0 ** -52


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _kinds():
    from tadmm._cabi import KIND_SVD, KIND_TT_CONV, KIND_TT_LINEAR
    return KIND_TT_CONV, KIND_TT_LINEAR, KIND_SVD


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _oracle(kind, zin, tts, ranks):
    """(Z of the oracle on `zin`, clamped rank list or None).  The oracle runs in float64 on the float32 values the
    kernel projects, so its own error is far below the bar."""
    conv, lin, _ = _kinds()
    z64 = zin.astype(np.float64)
    if kind == conv:
        r = list(ranks)
        return np.asarray(O.prune_conv_rank_tt(z64, tts, r)).reshape(zin.shape), r
    if kind == lin:
        r = list(ranks)
        O.ten2tt(np.zeros(tts, np.float32), tts, r)
        return np.asarray(O.prune_linear_rank_tt(z64, tts, list(ranks))).reshape(zin.shape), r
    z = O.prune_conv_rank_svd(z64, ranks) if zin.ndim == 4 else O.prune_linear_rank_svd(z64, ranks)
    return np.asarray(z).reshape(zin.shape), None


def _build(dev, cases, data, mis):
    """Layer dicts of one plan.  mis = (offW, offU, offZ); None = a plain `.clone()` (256-byte aligned)."""
    from _unaligned import SENTINEL, misaligned
    layers = []
    for (kind, shape, tts, ranks), (w, u) in zip(cases, data):
        t = dict(W=torch.from_numpy(w).to(dev), U=torch.from_numpy(u).to(dev),
                 Z=torch.full(shape, SENTINEL, dtype=torch.float32, device=dev))
        for key, off in zip(("W", "U", "Z"), mis):
            if off is not None:
                t[key] = misaligned(t[key], off)
            else:
                assert t[key].data_ptr() % 16 == 0
        L = dict(kind=kind, ranks=ranks, **t)
        if tts is not None:
            L["tt_shapes"] = tts
        layers.append(L)
    return layers


def _run(dev, cases, data, mis, update_u=True, use_u=True, skip_rotations=True):
    from tadmm import ops
    layers = _build(dev, cases, data, mis)
    plan = ops.ProjectionPlan(layers, skip_rotations=skip_rotations)
    resid = plan.run(update_u=update_u, use_u=use_u).cpu().numpy().copy()
    torch.cuda.synchronize()
    ranks = [list(r) for r in plan.ranks]
    plan.close()
    return layers, resid, ranks


def _check_host_arithmetic(cases, data, layers, resid, update_u=True):
    """U_out == U_in + (W - Z) in float32, bitwise; resid == sum((W - Z)^2) in fp64 up to the summation order; the
    guard elements around every misaligned view untouched."""
    from _unaligned import guards_intact
    for i, (L, (w, u)) in enumerate(zip(layers, data)):
        z = L["Z"].cpu().numpy()
        diff = w - z                                                         # one fp32 subtract per element
        want_u = u + diff if update_u else u                                 # one fp32 add per element
        assert np.array_equal(_bits(L["U"].cpu().numpy()), _bits(want_u)), cases[i]
        assert np.array_equal(_bits(L["W"].cpu().numpy()), _bits(w)), cases[i]
        want_r = float((diff.astype(np.float64) ** 2).sum())
        print(f"layer {i} {cases[i][1]}: resid {resid[i]!r} host {want_r!r}")
        assert abs(resid[i] - want_r) <= w.size * EPS64 * want_r, (cases[i], resid[i], want_r)
        for key in ("W", "U", "Z"):
            if L[key]._base is not None:
                assert guards_intact(L[key]), (cases[i], key)


def _check_oracle(cases, data, layers, ranks, refs, use_u=True):
    for i, (L, (w, u)) in enumerate(zip(layers, data)):
        zref, rref = refs[i]
        got = L["Z"].cpu().numpy()
        scale = float(np.abs(w + u if use_u else w).max())
        err = float(np.abs(got.astype(np.float64) - zref).max())
        print(f"layer {i} {cases[i][1]}: |Z - oracle| {err:.3e} = {err / scale:.3e} of max|W+U|")
        assert err <= BAR * scale, (cases[i], err, scale)
        if rref is not None:
            assert ranks[i] == rref, cases[i]                                 # bit-exact clamp


# ---------------------------------------------------------------------------------------------- A1
def _a1_cases():
    conv, lin, svd = _kinds()
    return [
        (lin, (30, 77), [2, 3, 5, 7, 11], [1, 2, 4, 6, 3, 1]),       # ragged flat layer
        (svd, (129, 131), None, 7),                                    # 16899 = 2 * 8192 + 515 elements, % 4 == 3
        (svd, (64, 257, 1, 1), None, [5]),                             # conv-shaped, K2 == 1
        (conv, (16, 16, 3, 3), [4, 4, 9, 4, 4], [1, 4, 12, 12, 4, 1]),  # shape-eligible for conv_vec<9>
        (conv, (6, 10, 5, 5), [6, 25, 10], [1, 3, 4, 1]),             # generic conv path
        (conv, (5, 3, 3, 3), [5, 9, 3], [1, 3, 2, 1]),
    ]


_A1 = {}


def _a1_data():
    if not _A1:
        rng = np.random.default_rng(2024)
        cases = _a1_cases()
        data = [(rng.standard_normal(c[1]).astype(np.float32), (0.3 * rng.standard_normal(c[1])).astype(np.float32))
                for c in cases]
        _A1["cases"], _A1["data"] = cases, data
        _A1["refs"] = [_oracle(c[0], w + u, c[2], c[3]) for c, (w, u) in zip(cases, data)]
        _A1["refs_w"] = [_oracle(c[0], w, c[2], c[3]) for c, (w, u) in zip(cases, data)]
    return _A1


_MIS = ([(o, None, None) for o in (1, 2, 3)] + [(None, o, None) for o in (1, 2, 3)] +
        [(None, None, o) for o in (1, 2, 3)] + [(1, 2, 3), (3, 1, 2), (None, None, None)])


@pytest.mark.parametrize("mis", _MIS, ids=lambda m: "W%sU%sZ%s" % tuple("-" if o is None else o for o in m))
def test_misaligned_operands_vs_oracle_and_aligned_twin(dev, mis):
    a1 = _a1_data()
    cases, data = a1["cases"], a1["data"]
    layers, resid, ranks = _run(dev, cases, data, mis)
    _check_oracle(cases, data, layers, ranks, a1["refs"])
    _check_host_arithmetic(cases, data, layers, resid)
    # aligned twin: a second plan instance over clones of the same data.  Unfold is an element-wise fp32 w + u and
    # fold a copy, identical in the vector and the scalar path; everything between them reads aligned scratch only.
    twin, resid_t, ranks_t = _run(dev, cases, data, (None, None, None))
    assert ranks == ranks_t
    for i, (L, T) in enumerate(zip(layers, twin)):
        assert torch.equal(L["Z"], T["Z"]), cases[i]
        assert torch.equal(L["U"], T["U"]), cases[i]
        assert abs(resid[i] - resid_t[i]) <= data[i][0].size * EPS64 * resid_t[i], (cases[i], resid[i], resid_t[i])


def test_misaligned_update_u_false_leaves_u_untouched(dev):
    a1 = _a1_data()
    layers, resid, ranks = _run(dev, a1["cases"], a1["data"], (1, 2, 3), update_u=False)
    _check_oracle(a1["cases"], a1["data"], layers, ranks, a1["refs"])
    _check_host_arithmetic(a1["cases"], a1["data"], layers, resid, update_u=False)      # U bitwise its input


def test_misaligned_use_u_false_projects_w_alone(dev):
    a1 = _a1_data()
    layers, resid, ranks = _run(dev, a1["cases"], a1["data"], (3, 1, 2), use_u=False)
    _check_oracle(a1["cases"], a1["data"], layers, ranks, a1["refs_w"], use_u=False)
    _check_host_arithmetic(a1["cases"], a1["data"], layers, resid)


# ---------------------------------------------------------------------------------------------- A2
# Chunking of the conv sweeps (csrc/plan.hip, layout_plan): ichunk = min(I, 512), halved while
# K2 * (ichunk + 4) > 12288; nchunk = ceil(I / ichunk).
#   (8, 1024, 3, 3): 9 * 516 = 4644          -> ichunk 512, chunks 512 + 512            (vector path, i0 = 512)
#   (8,  520, 3, 3):                          -> ichunk 512, chunks 512 + 8              (vector path, tiny last chunk)
#   (4, 1030, 3, 3): I % 4 != 0               -> ichunk 512, chunks 512 + 512 + 6        (generic path)
#   (4,  600, 5, 5): 25 * 516 = 12900 > 12288 -> ichunk 256, chunks 256 + 256 + 88       (generic path)
#   (4,  700, 7, 7): 49 * 260 = 12740 > 12288, 49 * 132 = 6468 -> ichunk 128, chunks 5 x 128 + 60
# TT modes (O, k^2, I) -- the first layer splits O and I further -- with at most 8 per bond, so every eigen-problem
# is small (N <= 196).  The inputs are Gaussian with a geometric scale along O and along the kernel position, which
# separates the singular values of every unfolding: the relative gap (s_r - s_{r+1}) / s_r at every kept bond is
# asserted >= 2 % on the host (`_bond_gaps`; the measured minimum over the five layers is stated there).
def _a2_cases():
    conv = _kinds()[0]
    return [
        (conv, (8, 1024, 3, 3), [2, 4, 9, 32, 32], [1, 2, 6, 8, 8, 1]),
        (conv, (8, 520, 3, 3), [8, 9, 520], [1, 5, 6, 1]),
        (conv, (4, 1030, 3, 3), [4, 9, 1030], [1, 3, 8, 1]),
        (conv, (4, 600, 5, 5), [4, 25, 600], [1, 3, 7, 1]),
        (conv, (4, 700, 7, 7), [4, 49, 700], [1, 2, 8, 1]),
    ]


def _a2_chunks(shape):
    """(ichunk, nchunk) by the sizing loop of layout_plan."""
    k2, i = shape[2] * shape[3], shape[1]
    ich = min(i, 512)
    while k2 * (ich + 4) > 12288 and ich > 1:
        ich //= 2
    return ich, -(-i // ich)


def _decaying(rng, shape, amp):
    o, i, kh, kw = shape
    g = rng.standard_normal(shape)
    g *= (0.62 ** np.arange(o))[:, None, None, None]
    g *= (0.87 ** np.arange(kh * kw)).reshape(1, 1, kh, kw)
    return (amp * g).astype(np.float32)


def _bond_gaps(zin, tts, ranks):
    """Relative gap (s_r - s_{r+1}) / s_r of every truncated unfolding of the TT-SVD of conv kernel `zin` (fp64)."""
    rest = O.conv_unfold(zin.astype(np.float64)).reshape(tts)
    r = list(ranks)
    gaps = []
    for i in range(len(tts) - 1):
        mat = rest.reshape(r[i] * tts[i], -1)
        u, s, vt = np.linalg.svd(mat, full_matrices=False)
        r[i + 1] = min(r[i + 1], s.shape[0])
        if r[i + 1] < s.shape[0]:
            gaps.append(float((s[r[i + 1] - 1] - s[r[i + 1]]) / s[r[i + 1] - 1]))
        rest = s[:r[i + 1], None] * vt[:r[i + 1]]
    return gaps


_A2 = {}


def _a2_data():
    if not _A2:
        rng = np.random.default_rng(77)
        cases = _a2_cases()
        data = [(_decaying(rng, c[1], 1.0), _decaying(rng, c[1], 0.25)) for c in cases]
        _A2["cases"], _A2["data"] = cases, data
        _A2["refs"] = [_oracle(c[0], w + u, c[2], c[3]) for c, (w, u) in zip(cases, data)]
    return _A2


def test_multichunk_chunking_is_what_the_cases_claim():
    """Host arithmetic only (still in this GPU file: it guards the comments above against a change of the sizing)."""
    got = [_a2_chunks(c[1]) for c in _a2_cases()]
    assert got == [(512, 2), (512, 2), (512, 3), (256, 3), (128, 6)], got


@pytest.mark.parametrize("off_w", [None, 1], ids=["aligned", "W1"])
def test_multichunk_conv_sweeps_vs_oracle(dev, off_w):
    a2 = _a2_data()
    cases, data = a2["cases"], a2["data"]
    for c, (w, u) in zip(cases, data):
        gaps = _bond_gaps(w + u, c[2], c[3])
        print(c[1], "bond gaps", ["%.3f" % g for g in gaps])
        assert min(gaps) >= 0.02, (c, gaps)           # precondition on the INPUT, not on the kernel (minimum: 0.025)
    layers, resid, ranks = _run(dev, cases, data, (off_w, None, None))
    _check_oracle(cases, data, layers, ranks, a2["refs"])
    _check_host_arithmetic(cases, data, layers, resid)


@pytest.mark.parametrize("off_w", [None, 1], ids=["aligned", "W1"])
def test_multichunk_full_rank_projection_is_the_identity_bitwise(dev, off_w):
    """Ranks at the clamp limit with FLAG_SKIP_ROTATIONS (the ProjectionPlan default): for modes (O, k^2, I) with
    O * k^2 <= I no unfolding is transposed and r == m at both steps, so build_geom marks every step `skip`, the
    plan runs unfold and fold back to back on one buffer, and Z must equal the fp32 sum W + U bit for bit -- the
    sharpest check of the i0 > 0 addressing of both transposes."""
    conv = _kinds()[0]
    a2 = _a2_data()
    cases = []
    for _, shape, _, _ in a2["cases"]:
        o, i, k2 = shape[0], shape[1], shape[2] * shape[3]
        assert o * k2 <= i                               # not transposed -> both steps are skipped rotations
        cases.append((conv, shape, [o, k2, i], [1, o, o * k2, 1]))
    layers, resid, ranks = _run(dev, cases, a2["data"], (off_w, None, None))
    for c, L, (w, u), r in zip(cases, layers, a2["data"], ranks):
        assert r == c[3], (c, r)
        assert np.array_equal(_bits(L["Z"].cpu().numpy()), _bits(w + u)), c[1]
    _check_host_arithmetic(cases, a2["data"], layers, resid)


# ---------------------------------------------------------------------------------------------- A3
SIZES = [7, 1, 8193, 3, 1000003, 5, 64 * 64 * 9]
# The big layers of SIZES start at concatenated offsets 8, 8204 and 1008212 -- multiples of 4 -- so a block that
# starts inside one of them starts on a multiple of 4 of the layer.  In SIZES_HEAD the layers of 8193 and 100003
# elements start at 7 and 8203: per = 112 elements per block, so their blocks start at layer offsets = 1 (mod 4)
# and run the scalar head [e0, v0) of penalty_kernel.
SIZES_HEAD = [7, 8193, 3, 100003, 5, 4099]


def _penalty_inputs(sizes, seed):
    rng = np.random.default_rng(seed)
    mk = lambda k, a: (a * rng.standard_normal(k)).astype(np.float32)      # noqa: E731
    return [mk(k, 1.0) for k in sizes], [mk(k, 0.9) for k in sizes], [mk(k, 0.3) for k in sizes]


def _penalty_ref(w, z, u, rho, gscale, loss_in, null=()):
    loss, grads = np.float64(loss_in), []
    acc = 0.0
    for i, (a, b, c) in enumerate(zip(w, z, u)):
        d = (a - b) + c                                                      # float32, the kernel's arithmetic
        acc += float((d.astype(np.float64) ** 2).sum())
        grads.append(None if i in null else np.float32(gscale) * d)
    return float(loss + 0.5 * np.float64(np.float32(rho)) * acc), grads


def _penalty_run(dev, w, z, u, offs, rho, gscale, loss_in=0.0, null=()):
    """One tadmm_penalty call on a pointer table built like ADMM._penalty_forward: [W.. | Z.. | U.. | G..].
    offs = (offW, offZ, offU, offG) misalignment in elements.  Returns (loss, gradient tensors or None)."""
    from _unaligned import SENTINEL, misaligned
    from tadmm import ops
    n = len(w)
    dt = [[misaligned(torch.from_numpy(x).to(dev), off) for x in arr] for arr, off in zip((w, z, u), offs[:3])]
    g = [None if i in null else
         misaligned(torch.full((len(w[i]),), SENTINEL, dtype=torch.float32, device=dev), offs[3]) for i in range(n)]
    ptrs = [t.data_ptr() for arr in dt for t in arr] + [0 if t is None else t.data_ptr() for t in g]
    ptrs_dev = torch.tensor(ptrs, dtype=torch.int64).to(dev)
    numel = [len(x) for x in w]
    numel_dev = torch.tensor(numel, dtype=torch.int64).to(dev)
    h = ops.Handle.get(dev.index)
    partial = torch.empty(h.lib.tadmm_penalty_scratch_doubles(), dtype=torch.float64, device=dev)
    loss = torch.full((1,), loss_in, dtype=torch.float64, device=dev)
    h.check(h.lib.tadmm_penalty(h.ptr, n, ptrs_dev.data_ptr(), numel_dev.data_ptr(), int(sum(numel)), float(rho),
                                float(gscale), loss.data_ptr(), partial.data_ptr(),
                                torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return float(loss.cpu()[0]), g, dt


def _penalty_check(dev, sizes, offs, rho=1e-3, gscale=None, loss_in=0.0, null=(), seed=5):
    from _unaligned import guards_intact
    gscale = rho if gscale is None else gscale
    w, z, u = _penalty_inputs(sizes, seed)
    want_loss, want_g = _penalty_ref(w, z, u, rho, gscale, loss_in, null)
    loss, g, dt = _penalty_run(dev, w, z, u, offs, rho, gscale, loss_in, null)
    total = sum(sizes)
    print(f"sizes {sizes} offs {offs}: loss {loss!r} host {want_loss!r} rel {abs(loss - want_loss) / abs(want_loss):.2e}")
    assert abs(loss - want_loss) <= total * EPS64 * abs(want_loss), (loss, want_loss)
    for i, (gt, gw) in enumerate(zip(g, want_g)):
        if gw is None:
            assert gt is None
            continue
        assert np.array_equal(_bits(gt.cpu().numpy()), _bits(gw)), (i, sizes[i])
        assert guards_intact(gt), (i, sizes[i])
    for arr, src in zip(dt, (w, z, u)):                                      # inputs are read-only
        for t, x in zip(arr, src):
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(x)) and guards_intact(t)
    return loss, g


@pytest.mark.parametrize("sizes", [SIZES, SIZES_HEAD], ids=["issue", "head"])
@pytest.mark.parametrize("offs", [(0, 0, 0, 0), (1, 2, 3, 0), (0, 0, 0, 1), (1, 2, 3, 2)],
                         ids=["aligned", "W1Z2U3", "G1", "W1Z2U3G2"])
def test_penalty_vs_numpy(dev, sizes, offs):
    _penalty_check(dev, sizes, offs)


def test_penalty_fewer_elements_than_blocks(dev):
    from tadmm import _cabi
    assert sum([1, 2, 3]) < _cabi.load().tadmm_penalty_scratch_doubles()
    _penalty_check(dev, [1, 2, 3], (0, 0, 0, 0))
    _penalty_check(dev, [1, 2, 3], (1, 2, 3, 1))


@pytest.mark.parametrize("sizes", [SIZES, SIZES_HEAD], ids=["issue", "head"])
@pytest.mark.parametrize("null", [(3,), (2,), "all"], ids=["small-middle", "big-middle", "all"])
def test_penalty_null_gradient_slots(dev, sizes, null):
    null = tuple(range(len(sizes))) if null == "all" else null
    full, _ = _penalty_check(dev, sizes, (0, 0, 0, 0))
    part, _ = _penalty_check(dev, sizes, (0, 0, 0, 0), null=null)
    assert part == full                                                       # the loss does not depend on the slots


@pytest.mark.parametrize("offs", [(0, 0, 0, 0), (1, 2, 3, 0)], ids=["aligned", "W1Z2U3"])
def test_penalty_grad_scale_and_accumulating_loss(dev, offs):
    _penalty_check(dev, SIZES_HEAD, offs, rho=1e-3, gscale=0.37, loss_in=2.5)
    _penalty_check(dev, SIZES, offs, rho=1e-3, gscale=0.37, loss_in=-1.0e3)


def test_penalty_is_deterministic(dev):
    a, ga = _penalty_check(dev, SIZES, (1, 2, 3, 0))
    b, gb = _penalty_check(dev, SIZES, (1, 2, 3, 0))
    assert a == b
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)
